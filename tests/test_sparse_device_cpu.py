"""CPU: the device CSR entry without a GPU - the export and the Fortran door exist, the Fortran program that hands device arrays to
engine_set_sparse_device compiles and links, and the torch front ends check dtype, layout and device before any library call."""
import os
import subprocess

import numpy as np
import pytest
import torch

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import CEngine, device_csr_tensors, is_torch_csr
from test_fortran_programs import FC, LIBDIR, MODDIR, SRC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_sparse_device_program(workdir):
    """prog_sparse_device links the HIP runtime itself (its hipMalloc / hipMemcpy interfaces)"""
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "prog_sparse_device")
    cmd = [FC, "-O1", "-fopenmp=libiomp5", f"-I{MODDIR}", "-module-dir", str(workdir), os.path.join(SRC, "prog_sparse_device.f90"),
           f"-L{LIBDIR}", "-lfortran_davidson_amd", "-ldavidson_hip", f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/conda/lib", "-Wl,-rpath,/opt/conda/lib", "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=workdir)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def test_the_entry_and_the_fortran_door_are_exported():
    assert hasattr(fd.hip_lib(), "dav_set_operator_csr_dev")
    assert hasattr(fd.fortran_lib(), "fd_engine_set_sparse_device")
    hdr = open(os.path.join(ROOT, "include", "davidson_hip.h")).read()
    assert "int dav_set_operator_csr_dev(" in hdr
    f90 = open(os.path.join(ROOT, "fortran_davidson_amd", "fortran", "davidson_hip_c.f90")).read()
    assert 'bind(C, name="dav_set_operator_csr_dev")' in f90


@pytest.mark.skipif(not os.path.exists(FC), reason="flang not available")
def test_sparse_device_program_compiles_and_links(tmp_path):
    assert os.path.exists(build_sparse_device_program(tmp_path))


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


def _parts(n=4):
    return torch.tensor([0, 1, 2, 3, 4]), torch.arange(n), torch.ones(n, dtype=torch.float64)


def test_torch_layout_is_recognised():
    rp, ci, vv = _parts()
    assert is_torch_csr(torch.sparse_csr_tensor(rp, ci, vv, size=(4, 4)))
    assert not is_torch_csr(vv) and not is_torch_csr(np.zeros(3))


@pytest.mark.parametrize("which,bad", [(0, torch.float64), (1, torch.int16), (2, torch.float32), (2, torch.int64)])
def test_dtypes_are_refused_before_any_call(which, bad):
    parts = list(_parts())
    parts[which] = parts[which].to(bad)
    with pytest.raises(TypeError):
        _engine(4).set_operator_csr_dev(0, *parts)


def test_host_tensors_and_numpy_arrays_are_refused_for_the_device_entry():
    with pytest.raises(ValueError, match="lies on cpu"):
        _engine(4).set_operator_csr_dev(0, *_parts())
    rp, ci, vv = _parts()
    with pytest.raises(TypeError, match="must be a torch tensor"):
        _engine(4).set_operator_csr_dev(0, rp.numpy(), ci, vv)
    with pytest.raises(ValueError, match="contiguous"):
        device_csr_tensors(rp, torch.arange(8)[::2], vv, 4, 0)


def test_a_cpu_torch_csr_tensor_takes_the_host_path(monkeypatch):
    rp, ci, vv = _parts()
    seen = {}

    class Lib(_NoCalls):
        def dav_set_operator_csr(self, h, which, rp, ci, vv, base, tri):
            seen["host"] = True
            return 0

    e = _engine(4)
    e.lib = Lib()
    e.set_operator_csr(0, torch.sparse_csr_tensor(rp, ci, vv, size=(4, 4)))
    assert seen == {"host": True}
