"""CPU: the device BSR entry without a GPU - the export and the Fortran door exist, the Fortran program that hands device block arrays
to engine_set_block_sparse_device compiles and links, the torch front ends check dtype, shape, layout, device and lengths before any
library call, and a torch BSR tensor is told from a CSR one."""
import os
import subprocess

import numpy as np
import pytest
import torch

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import CEngine, device_bsr_tensors, is_torch_bsr, is_torch_csr, torch_bsr_parts
from test_fortran_programs import FC, LIBDIR, MODDIR, SRC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_bsr_device_program(workdir):
    """prog_bsr_device links the HIP runtime itself (its hipMalloc / hipMemcpy interfaces)"""
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "prog_bsr_device")
    cmd = [FC, "-O1", "-fopenmp=libiomp5", f"-I{MODDIR}", "-module-dir", str(workdir), os.path.join(SRC, "prog_bsr_device.f90"),
           f"-L{LIBDIR}", "-lfortran_davidson_amd", "-ldavidson_hip", f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/conda/lib", "-Wl,-rpath,/opt/conda/lib", "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=workdir)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def test_the_entry_and_the_fortran_door_are_exported():
    assert hasattr(fd.hip_lib(), "dav_set_operator_bsr_dev")
    assert hasattr(fd.fortran_lib(), "fd_engine_set_block_sparse_device")
    hdr = open(os.path.join(ROOT, "include", "davidson_hip.h")).read()
    assert "int dav_set_operator_bsr_dev(" in hdr
    assert "#define DAV_HIP_ABI_VERSION 109" in hdr and fd.hip_lib().dav_version() == 109          # additive: the ABI stays
    f90 = open(os.path.join(ROOT, "fortran_davidson_amd", "fortran", "davidson_hip_c.f90")).read()
    assert 'bind(C, name="dav_set_operator_bsr_dev")' in f90
    sparse = open(os.path.join(ROOT, "fortran_davidson_amd", "fortran", "davidson_sparse.f90")).read()
    assert "engine_set_block_sparse_device" in sparse.split("contains")[0]          # public


@pytest.mark.skipif(not os.path.exists(FC), reason="flang not available")
def test_bsr_device_program_compiles_and_links(tmp_path):
    assert os.path.exists(build_bsr_device_program(tmp_path))


class _NoCalls:
    """a library stand-in whose every symbol fails the test when called"""
    def __getattr__(self, name):
        def call(*args):
            raise AssertionError(f"{name} was called")
        return call


def _engine(n):
    e = CEngine.__new__(CEngine)
    e.lib, e.h, e.n, e.device, e.owned = _NoCalls(), None, n, 0, False
    return e


def _parts(nb=4, b=2):
    """block diagonal: nb blocks of b x b"""
    return torch.arange(nb + 1), torch.arange(nb), torch.ones((nb, b, b), dtype=torch.float64)


def test_torch_layouts_are_told_apart():
    rp, ci, vv = _parts()
    bsr = torch.sparse_bsr_tensor(rp, ci, vv, size=(8, 8))
    csr = torch.sparse_csr_tensor(rp, ci, torch.ones(4, dtype=torch.float64), size=(4, 4))
    assert is_torch_bsr(bsr) and not is_torch_csr(bsr)
    assert is_torch_csr(csr) and not is_torch_bsr(csr)
    assert not is_torch_bsr(vv) and not is_torch_bsr(np.zeros(3))
    p = torch_bsr_parts(bsr)
    assert all(isinstance(x, np.ndarray) for x in p) and p[2].shape == (4, 2, 2)
    with pytest.raises(ValueError, match="square"):
        torch_bsr_parts(torch.sparse_bsr_tensor(rp, ci, vv, size=(8, 10)))


@pytest.mark.parametrize("which,bad", [(0, torch.float64), (1, torch.int16), (2, torch.float32), (2, torch.int64)])
def test_dtypes_are_refused_before_any_call(which, bad):
    parts = list(_parts())
    parts[which] = parts[which].to(bad)
    with pytest.raises(TypeError):
        _engine(8).set_operator_bsr_dev(0, *parts)


def test_host_tensors_and_numpy_arrays_are_refused_for_the_device_entry():
    with pytest.raises(ValueError, match="lies on cpu"):
        _engine(8).set_operator_bsr_dev(0, *_parts())
    rp, ci, vv = _parts()
    with pytest.raises(TypeError, match="must be a torch tensor"):
        _engine(8).set_operator_bsr_dev(0, rp.numpy(), ci, vv)
    with pytest.raises(ValueError, match="contiguous"):
        device_bsr_tensors(rp, torch.arange(8)[::2], vv, 8, 0)
    with pytest.raises(ValueError, match="contiguous"):
        device_bsr_tensors(rp, ci, vv.transpose(1, 2)[:, :, :1].expand(4, 2, 2), 8, 0)


class _OnDevice(torch.Tensor):
    """a CPU tensor that says it lies on cuda:0 - the checks behind the device check can run without a GPU"""
    @property
    def device(self):
        return torch.device("cuda", 0)


def _fake(t):
    return t.as_subclass(_OnDevice)


def test_shapes_and_lengths_are_refused_before_any_call():
    rp, ci, vv = (_fake(t) for t in _parts())
    e = _engine(8)
    for args, msg in [((rp, ci, _fake(torch.ones(4, 4, dtype=torch.float64))), "3 dimensions"),
                      ((rp, ci, _fake(torch.ones(4, 2, 3, dtype=torch.float64))), r"shape \(nnzb, b, b\)"),
                      ((rp, ci, _fake(torch.ones(4, 17, 17, dtype=torch.float64))), "must lie in 1..16"),
                      ((rp, ci, _fake(torch.ones(4, 3, 3, dtype=torch.float64))), "not a multiple"),
                      ((_fake(torch.arange(4)), ci, vv), r"n / b \+ 1 = 5 offsets"),
                      ((rp, _fake(torch.arange(3)), vv), "row_ptr says 4 blocks"),
                      ((rp, ci, _fake(torch.ones(3, 2, 2, dtype=torch.float64))), "row_ptr says 4 blocks"),
                      ((_fake(torch.arange(5).reshape(5, 1)), ci, vv), "contiguous tensor of 1 dimension")]:
        with pytest.raises(ValueError, match=msg):
            e.set_operator_bsr_dev(0, *args)
    assert device_bsr_tensors(rp, _fake(torch.arange(4, dtype=torch.int32)), vv, 8, 0) == (2, 64, 32)


def test_a_cpu_torch_bsr_tensor_takes_the_host_path():
    rp, ci, vv = _parts()
    seen = {}

    class Lib(_NoCalls):
        def dav_set_operator_bsr(self, h, which, b, rp, ci, vv, base, tri, layout):
            seen["host"] = (b, layout)
            return 0

    e = _engine(8)
    e.lib = Lib()
    e.set_operator_bsr(0, torch.sparse_bsr_tensor(rp, ci, vv, size=(8, 8)))
    assert seen == {"host": (2, 0)}
