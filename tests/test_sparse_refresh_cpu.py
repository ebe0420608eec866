"""CPU: new values on a kept pattern without a GPU - the three entries and the three Fortran doors are exported by both libraries and
known to the Python mirror of the ABI, the Fortran program that updates a csr_matrix compiles and links, and the front ends check dtype
and length before any engine call."""
import os
import subprocess

import numpy as np
import pytest
import torch

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import CEngine, DavidsonHipError, update_values_array
from test_fortran_programs import FC, LIBDIR, MODDIR, SRC, compile_link

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dav_keep_value_map", "dav_update_operator_values", "dav_update_operator_values_dev")
DOORS = ("fd_engine_keep_value_map", "fd_engine_update_values", "fd_engine_update_values_device")


def build_sparse_refresh_program(workdir):
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    return compile_link([os.path.join(SRC, "prog_sparse_refresh.f90")], os.path.join(bindir, "prog_sparse_refresh"), workdir)


def test_the_entries_and_the_fortran_doors_are_exported():
    product = os.path.join(LIBDIR, "libdavidson_hip.so")
    names = subprocess.run(["nm", "-D", "--defined-only", product], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "davidson_hip.h")).read()
    f90 = open(os.path.join(ROOT, "fortran_davidson_amd", "fortran", "davidson_hip_c.f90")).read()
    for name in ENTRIES:
        assert hasattr(fd.hip_lib(), name), name            # the library pytest loads (the test build)
        assert f" T {name}\n" in names, name                # the product
        assert f"int {name}(" in hdr
        assert f'bind(C, name="{name}")' in f90
    for name in DOORS:
        assert hasattr(fd.fortran_lib(), name), name
    for method in ("keep_value_map", "update_operator_values"):
        assert callable(getattr(CEngine, method))
    for method in ("update_values",):
        assert callable(getattr(fd.DavidsonEngine, method))


@pytest.mark.skipif(not os.path.exists(FC), reason="flang not available")
def test_sparse_refresh_program_compiles_and_links(tmp_path):
    if not os.path.isdir(MODDIR):
        pytest.skip("module files not built")
    assert os.path.exists(build_sparse_refresh_program(tmp_path))


class _NoCalls:
    """a library stand-in whose every symbol fails the test when called"""
    def __getattr__(self, name):
        def call(*args):
            raise AssertionError(f"{name} was called")
        return call


def _engine(n, count):
    e = CEngine.__new__(CEngine)
    e.lib, e.h, e.n, e.device, e.owned = _NoCalls(), None, n, 0, False
    e._saw_values(0, count)
    return e


@pytest.mark.parametrize("bad", [np.float32, np.int64, np.complex128])
def test_numpy_dtypes_are_refused_before_any_call(bad):
    with pytest.raises(TypeError, match="expected float64"):
        _engine(4, 6).update_operator_values(0, np.ones(6, dtype=bad))


@pytest.mark.parametrize("bad", [torch.float32, torch.int64])
def test_torch_dtypes_are_refused_before_any_call(bad):
    with pytest.raises(TypeError, match="expected torch.float64"):
        _engine(4, 6).update_operator_values(0, torch.ones(6, dtype=bad))


def test_a_wrong_length_is_refused_before_any_call():
    for vals in (np.ones(5), np.ones(7), np.ones((2, 2, 2)), torch.ones(5, dtype=torch.float64)):
        with pytest.raises(ValueError, match="the set call saw 6 values"):
            _engine(4, 6).update_operator_values(0, vals)
    with pytest.raises(ValueError, match="contiguous"):
        _engine(4, 6).update_operator_values(0, torch.ones(12, dtype=torch.float64)[::2])


def test_blocks_are_taken_flat_or_as_nnzb_b_b_and_reach_the_host_entry():
    seen = []

    class Lib(_NoCalls):
        def dav_update_operator_values(self, h, which, vals):
            seen.append(which)
            return 0

    e = _engine(4, 8)
    e.lib = Lib()
    e.update_operator_values(0, np.arange(8.0))
    e.update_operator_values(0, np.arange(8.0).reshape(2, 2, 2))
    e.update_operator_values(0, torch.arange(8, dtype=torch.float64))        # a CPU tensor is host data
    assert seen == [0, 0, 0]
    flat, dev = update_values_array(np.arange(8.0).reshape(2, 2, 2), 8)
    assert dev is None and flat.shape == (8,) and np.array_equal(flat, np.arange(8.0))


def test_update_values_checks_before_the_fortran_doors():
    """DavidsonEngine.update_values: the host door stops the process on an engine error, so everything is checked in Python first"""
    eng = fd.DavidsonEngine.__new__(fd.DavidsonEngine)
    eng.n, eng.lib, eng.p, eng.device = 30, _NoCalls(), None, 0
    with pytest.raises(DavidsonHipError, match="dav_keep_value_map"):
        eng.update_values(1, np.ones(10))
    eng._kept = {1: {"count": 10, "b": 1, "fortran_blocks": False}, 2: {"count": 8, "b": 2, "fortran_blocks": True}}
    with pytest.raises(ValueError, match="the set call saw 10 values"):
        eng.update_values(1, np.ones(11))
    with pytest.raises(TypeError):
        eng.update_values(1, np.ones(10, dtype=np.float32))
    with pytest.raises(TypeError):
        eng.update_values(2, torch.ones(8, dtype=torch.float32))


def test_update_values_hands_the_fortran_door_blocks_in_fortran_order():
    got = {}

    class Lib(_NoCalls):
        def fd_engine_update_values(self, p, which, vals, count):
            got["which"], got["vals"] = which, np.ctypeslib.as_array(vals, shape=(count,)).copy()

    eng = fd.DavidsonEngine.__new__(fd.DavidsonEngine)
    eng.n, eng.lib, eng.p, eng.device = 4, Lib(), None, 0
    eng._kept = {2: {"count": 8, "b": 2, "fortran_blocks": True}}
    blocks = np.arange(8.0).reshape(2, 2, 2)                                 # row-major blocks, as set_block_sparse takes them
    eng.update_values(2, blocks)
    assert got["which"] == 2 and np.array_equal(got["vals"], blocks.transpose(0, 2, 1).reshape(-1))
