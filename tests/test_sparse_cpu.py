"""CPU: the sparse (CSR) operator without a GPU - the Fortran program that solves a csr_matrix through the generic compiles and links
against the modules, the ABI mirrors know the new entry point, and the Python wrappers refuse malformed CSR input before any engine
call (no engine is created here)."""
import os
import re

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import DavidsonHipError, check_csr, csr_arrays
from test_fortran_programs import FC, SRC, compile_link

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def banded(n, lower=False):
    rows, cols, vals = [], [], []
    for i in range(n):
        for j in range(max(0, i - 2), (i if lower else min(n - 1, i + 2)) + 1):
            rows.append(i)
            cols.append(j)
            vals.append(1.0 + i if i == j else 0.1)
    indptr = np.searchsorted(np.array(rows), np.arange(n + 1))
    return indptr.astype(np.int64), np.array(cols, dtype=np.int32), np.array(vals)


@pytest.mark.skipif(not os.path.exists(FC), reason="flang not available")
def test_sparse_program_compiles_and_links(tmp_path):
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    exe = compile_link([os.path.join(SRC, "prog_sparse.f90")], os.path.join(bindir, "prog_sparse"), tmp_path)
    assert os.path.exists(exe)


def test_abi_mirrors_know_the_csr_entry():
    hdr = open(os.path.join(ROOT, "include", "davidson_hip.h")).read()
    assert "dav_set_operator_csr" in hdr and "DAV_CSR_LOWER = 1" in hdr
    assert hasattr(fd.hip_lib(), "dav_set_operator_csr")
    f90 = open(os.path.join(ROOT, "fortran_davidson_amd", "fortran", "davidson_hip_c.f90")).read()
    assert 'name="dav_set_operator_csr"' in f90
    assert int(re.search(r"DAV_HIP_ABI_VERSION = (\d+)", f90).group(1)) == fd.engine_c.ABI_VERSION == 109
    lib = fd.fortran_lib()
    for name in ("fd_engine_set_sparse", "fd_sparse_solve"):
        assert hasattr(lib, name), name


def test_a_valid_matrix_passes_the_checks():
    n = 50
    rp, ci, vv = check_csr(*banded(n), n)
    assert rp.dtype == np.int64 and ci.dtype == np.int32 and vv.dtype == np.float64
    check_csr(*banded(n, lower=True), n, lower=True)
    rp1, ci1, vv1 = banded(n)
    check_csr(rp1 + 1, ci1 + 1, vv1, n, base=1)


class _FakeScipy:
    """what the wrappers read of a scipy sparse matrix: .tocsr() with indptr / indices / data (scipy is not imported)"""
    def __init__(self, rp, ci, vv):
        self.indptr, self.indices, self.data = rp, ci, vv

    def tocsr(self):
        return self


def test_an_object_with_tocsr_is_accepted():
    rp, ci, vv = csr_arrays(_FakeScipy(*banded(20)), n=20)
    assert rp.size == 21 and ci.size == vv.size == rp[-1]


@pytest.mark.parametrize("case", ["short_indptr", "short_indices", "short_data", "non_monotone", "col_negative", "col_too_large",
                                  "upper_with_lower", "indptr_not_at_base"])
def test_malformed_input_is_refused_before_any_engine_call(case, monkeypatch):
    n = 40
    rp, ci, vv = banded(n)
    lower = False
    if case == "short_indptr":
        rp = rp[:-1]
    elif case == "short_indices":
        ci = ci[:-3]
    elif case == "short_data":
        vv = vv[:-1]
    elif case == "non_monotone":
        rp = rp.copy()
        rp[7] = rp[9]
    elif case == "col_negative":
        ci = ci.copy()
        ci[5] = -1
    elif case == "col_too_large":
        ci = ci.copy()
        ci[-1] = n
    elif case == "upper_with_lower":
        lower = True
    elif case == "indptr_not_at_base":
        rp = rp + 1
    # no engine exists and none may be created: the Fortran doors must never be reached
    calls = []
    monkeypatch.setattr(fd.solver, "fortran_lib", lambda: calls.append(1) or pytest.fail("engine door called"))
    with pytest.raises(ValueError):
        check_csr(rp, ci, vv, n, lower=lower)
    with pytest.raises(ValueError):
        fd.generalized_eigensolver_sparse(rp, ci, vv, 3, "DPR", 100, 1e-8, lower=lower)
    assert not calls


def test_set_sparse_refuses_before_the_fortran_door():
    """DavidsonEngine.set_sparse checks the arrays in Python first: the Fortran door stops the process on an engine error"""
    class NoDoor:
        def __getattr__(self, name):
            pytest.fail(f"{name} called with malformed input")
    eng = fd.DavidsonEngine.__new__(fd.DavidsonEngine)
    eng.n, eng.lib, eng.p = 30, NoDoor(), None
    rp, ci, vv = banded(30)
    with pytest.raises(ValueError):
        eng.set_sparse(1, rp, ci, vv, lower=True)
    with pytest.raises(ValueError):
        eng.set_sparse(1, rp[:-2], ci, vv)


def test_cengine_length_checks_raise_the_engine_error():
    """CEngine.set_operator_csr hands everything else to the engine's validation, but never lets C read past the arrays"""
    rp, ci, vv = banded(30)
    with pytest.raises(DavidsonHipError, match="offsets"):
        csr_arrays(rp[:-1], ci, vv, 30)
    with pytest.raises(DavidsonHipError, match="entries"):
        csr_arrays(rp, ci[:5], vv, 30)
