"""CPU: the block-sparse (BSR) operator without a GPU - the Fortran program that solves a bsr_matrix through the generic compiles and links
against the modules, the ABI mirrors and the Fortran library know the new entry point and doors, and the Python checks refuse malformed
BSR input before any engine call (no engine is created here)."""
import os
import re

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import BSR_COL_MAJOR, DavidsonHipError, bsr_arrays, check_bsr
from test_fortran_programs import FC, SRC, compile_link

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def block_banded(nb, b, lower=False):
    """block-tridiagonal symmetric matrix: (indptr, indices, data (nnzb, b, b))"""
    bi, bj, blk = [], [], []
    for I in range(nb):
        for J in range(max(0, I - 1), (I if lower else min(nb - 1, I + 1)) + 1):
            bi.append(I)
            bj.append(J)
            blk.append(np.eye(b) * (1.0 + I) if I == J else np.full((b, b), 0.1))
    indptr = np.searchsorted(np.array(bi), np.arange(nb + 1))
    return indptr.astype(np.int64), np.array(bj, dtype=np.int32), np.array(blk)


@pytest.mark.skipif(not os.path.exists(FC), reason="flang not available")
def test_bsr_program_compiles_and_links(tmp_path):
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    exe = compile_link([os.path.join(SRC, "prog_bsr.f90")], os.path.join(bindir, "prog_bsr"), tmp_path)
    assert os.path.exists(exe)


def test_abi_mirrors_know_the_bsr_entry():
    hdr = open(os.path.join(ROOT, "include", "davidson_hip.h")).read()
    assert "int dav_set_operator_bsr(" in hdr and "DAV_BSR_COL_MAJOR = 1" in hdr
    assert "#define DAV_HIP_ABI_VERSION 109" in hdr
    assert hasattr(fd.hip_lib(), "dav_set_operator_bsr")
    f90 = open(os.path.join(ROOT, "fortran_davidson_amd", "fortran", "davidson_hip_c.f90")).read()
    assert 'name="dav_set_operator_bsr"' in f90 and "DAV_BSR_COL_MAJOR = 1" in f90
    assert int(re.search(r"DAV_HIP_ABI_VERSION = (\d+)", f90).group(1)) == fd.engine_c.ABI_VERSION == 109


def test_fortran_library_exports_the_bsr_doors():
    lib = fd.fortran_lib()
    for name in ("fd_engine_set_block_sparse", "fd_bsr_solve", "fd_engine_set_sparse", "fd_sparse_solve"):
        assert hasattr(lib, name), name


def test_a_valid_matrix_passes_the_checks():
    nb, b = 12, 4
    n = nb * b
    bs, rp, ci, vv = check_bsr(*block_banded(nb, b), n)
    assert bs == b and rp.dtype == np.int64 and ci.dtype == np.int32 and vv.dtype == np.float64 and vv.shape[1:] == (b, b)
    check_bsr(*block_banded(nb, b, lower=True), n, lower=True)
    rp1, ci1, vv1 = block_banded(nb, b)
    check_bsr(rp1 + 1, ci1 + 1, vv1, n, base=1, layout=BSR_COL_MAJOR)


class _FakeBsr:
    """what the wrappers read of a scipy bsr_matrix: .indptr, .indices, .data (nnzb, b, b) and .blocksize (scipy is not imported)"""
    def __init__(self, rp, ci, vv):
        self.indptr, self.indices, self.data = rp, ci, vv
        self.blocksize = vv.shape[1:]


def test_a_duck_typed_bsr_object_is_accepted():
    nb, b = 10, 3
    bs, rp, ci, vv = bsr_arrays(_FakeBsr(*block_banded(nb, b)), n=nb * b)
    assert bs == b and rp.size == nb + 1 and ci.size == vv.shape[0] == rp[-1]
    bs, *_ = check_bsr(_FakeBsr(*block_banded(nb, b)), None, None, nb * b)
    assert bs == b


def test_a_scipy_bsr_matrix_is_accepted():
    sp = pytest.importorskip("scipy.sparse")
    nb, b = 8, 4
    rp, ci, vv = block_banded(nb, b)
    m = sp.bsr_matrix((vv, ci, rp), shape=(nb * b, nb * b))
    bs, rp2, ci2, vv2 = check_bsr(m, None, None, nb * b)
    assert bs == b and np.array_equal(rp2, rp) and np.array_equal(vv2, vv)


@pytest.mark.parametrize("case", ["n_not_multiple", "b_zero", "b_17", "non_monotone", "col_negative", "col_too_large", "upper_with_lower",
                                  "indptr_not_at_base", "bad_layout", "bad_base", "short_indptr", "short_data", "non_square"])
def test_malformed_input_is_refused_before_any_engine_call(case, monkeypatch):
    nb, b = 10, 4
    n = nb * b
    rp, ci, vv = block_banded(nb, b)
    kw = {}
    if case == "n_not_multiple":
        n = n + 2
    elif case == "b_zero":
        vv = np.zeros((vv.shape[0], 0, 0))
    elif case == "b_17":
        vv = np.zeros((vv.shape[0], 17, 17))
        n = 17 * nb
    elif case == "non_monotone":
        rp = rp.copy()
        rp[4] = rp[6]
    elif case == "col_negative":
        ci = ci.copy()
        ci[5] = -1
    elif case == "col_too_large":
        ci = ci.copy()
        ci[-1] = nb
    elif case == "upper_with_lower":
        kw["lower"] = True
    elif case == "indptr_not_at_base":
        rp = rp + 1
    elif case == "bad_layout":
        kw["layout"] = 2
    elif case == "bad_base":
        kw["base"] = 2
    elif case == "short_indptr":
        rp = rp[:-1]
    elif case == "short_data":
        vv = vv[:-1]
    elif case == "non_square":
        vv = np.zeros((vv.shape[0], 4, 2))
    calls = []
    monkeypatch.setattr(fd.solver, "fortran_lib", lambda: calls.append(1) or pytest.fail("engine door called"))
    with pytest.raises(ValueError):
        check_bsr(rp, ci, vv, n, **kw)
    if "layout" not in kw and "base" not in kw:
        with pytest.raises(ValueError):
            fd.generalized_eigensolver_bsr(rp, ci, vv, 3, "DPR", 100, 1e-8, lower=kw.get("lower", False), n=n)
    assert not calls


def test_set_block_sparse_refuses_before_the_fortran_door():
    """DavidsonEngine.set_block_sparse checks the arrays in Python first: the Fortran door stops the process on an engine error"""
    class NoDoor:
        def __getattr__(self, name):
            pytest.fail(f"{name} called with malformed input")
    eng = fd.DavidsonEngine.__new__(fd.DavidsonEngine)
    eng.n, eng.lib, eng.p = 40, NoDoor(), None
    rp, ci, vv = block_banded(10, 4)
    with pytest.raises(ValueError):
        eng.set_block_sparse(1, rp, ci, vv, lower=True)
    with pytest.raises(ValueError):
        eng.set_block_sparse(1, rp[:-2], ci, vv)


def test_cengine_length_checks_raise_the_engine_error():
    """CEngine.set_operator_bsr hands the rest to the engine's validation, but never lets C read past the arrays"""
    rp, ci, vv = block_banded(10, 4)
    with pytest.raises(DavidsonHipError, match="offsets"):
        bsr_arrays(rp[:-1], ci, vv, 40)
    with pytest.raises(DavidsonHipError, match="blocks"):
        bsr_arrays(rp, ci[:5], vv, 40)
