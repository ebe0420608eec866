"""CPU: complex Hermitian CSR operators exist in every layer.  They are extension entries next to ABI 109 (include/davidson_hip_herm.h,
prefix davh_; doors prefix fdh_): both builds of the engine export exactly davh_set_operator_csr(_dev) and the Fortran library the two
doors; the four mirrors - header, ctypes tables, Fortran interface module, doors - are compared the way tests/test_coo_cpu.py compares
its own; davidson_hip.h and davidson_hip_ext.h are byte for byte what they were; the extraction of the complex pairs holds on numpy
real-form pairs (generic, pencil, a cluster across the cut); and the array extraction hands over scipy and torch complex input as it
stands, without a copy or an expansion of the values."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import fortran_davidson_amd as fd
import herm_inputs as H
from fortran_davidson_amd import _abi, engine_c, solver
from test_abi_cpu import C_API_F90, HIP_C_F90, as_fortran_sees, c_class, fortran_procedures, mismatches, read, strip_c_comments, table_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fortran_davidson_amd", "lib")
HERM_H = os.path.join(ROOT, "include", "davidson_hip_herm.h")
ENTRIES = {"davh_set_operator_csr", "davh_set_operator_csr_dev"}
DOORS = {"fdh_engine_set_hermitian", "fdh_engine_set_hermitian_device"}
# sha256 of the two headers this feature must leave alone
PINNED = {"davidson_hip.h": "606887b8d2ed27ae27f2e16a902484e205e631424ad00ea8503e23a662044850",
          "davidson_hip_ext.h": "012fff7744a002271859fd919016374ff0414168539494905ed426d19c352b09"}


def exported(lib, prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return set(re.findall(rf"\s[TW]\s+({prefix}\w+)$", out, re.M))


def herm_prototypes():
    return {name: ("i32", tuple(c_class(a.strip()) for a in args.split(",")))
            for name, args in re.findall(r"\bint\s+(davh_\w+)\s*\(([^()]*)\)\s*;", strip_c_comments(read(HERM_H)))}


def test_both_libraries_export_the_entries_and_the_doors():
    for lib in (os.path.join(LIBDIR, "libdavidson_hip.so"), os.path.join(LIBDIR, "test", "libdavidson_hip.so")):
        assert exported(lib, "davh_") == ENTRIES, lib
    assert exported(os.path.join(LIBDIR, "libfortran_davidson_amd.so"), "fdh_") == DOORS
    syms = subprocess.run(["strings", os.path.join(LIBDIR, "libdavidson_hip.so")], capture_output=True, text=True, check=True).stdout
    for kernel in ("bsr_build_gather_pairs_kernel", "bsr_build_diag_pairs_kernel", "bsr_refresh_diag_pairs_kernel"):
        assert kernel in syms, kernel


def test_the_four_mirrors_are_equal():
    header = herm_prototypes()
    assert set(header) == ENTRIES
    assert header["davh_set_operator_csr"] == ("i32", ("ptr", "i32", "ptr", "ptr", "ptr", "i32", "i32"))
    assert header["davh_set_operator_csr_dev"] == ("i32", ("ptr", "i32", "ptr", "i32", "ptr", "i32", "ptr", "i32", "i32"))
    assert mismatches(header, table_signatures(_abi.HERM)) == []
    assert mismatches(header, fortran_procedures(read(HIP_C_F90), "davh_"), see=as_fortran_sees) == []
    doors = fortran_procedures(read(C_API_F90), "fdh_")
    assert set(doors) == DOORS and mismatches(doors, table_signatures(_abi.HERM_FD)) == []
    for table in (_abi.HERM, _abi.HERM_FD):
        assert not set(table) & (set(_abi.DAV) | set(_abi.FD) | set(_abi.EXT) | set(_abi.EXT_FD))
    pkg = os.path.join(ROOT, "fortran_davidson_amd")
    called = {name for f in os.listdir(pkg) if f.endswith(".py") for name in re.findall(r"\.((?:davh|fdh)_\w+)\(", read(os.path.join(pkg, f)))}
    assert called == ENTRIES | DOORS


def test_the_two_existing_headers_are_untouched():
    for name, digest in PINNED.items():
        with open(os.path.join(ROOT, "include", name), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == digest, name
    assert re.search(r"#define\s+DAV_HIP_ABI_VERSION\s+109\b", read(os.path.join(ROOT, "include", "davidson_hip.h")))


def test_the_front_ends_exist():
    assert callable(fd.generalized_eigensolver_hermitian) and callable(fd.hermitian_eigenpairs)
    assert callable(fd.DavidsonEngine.set_hermitian)
    assert callable(fd.CEngine.set_operator_csr_hermitian) and callable(fd.CEngine.set_operator_csr_hermitian_dev)


# ---- the extraction -----------------------------------------------------------------------------------------------------------------
def real_pairs(h, s, lowest, eps=0.0, seed=0):
    """the 2 * lowest lowest real-form pairs as eigh gives them - an arbitrary rotation inside every double eigenvalue - or (eps > 0)
    the Ritz pairs of that span perturbed by eps, S-orthonormal: what a solver stopped at a residual of about eps hands over"""
    sl = pytest.importorskip("scipy.linalg")
    a, b = H.real_form(h), None if s is None else H.real_form(s)
    theta, v = sl.eigh(a, b)
    theta, v = theta[:2 * lowest], v[:, :2 * lowest]
    if eps > 0.0:
        q = v + eps * np.random.default_rng(seed).standard_normal(v.shape)
        theta, y = sl.eigh(q.T @ a @ q, q.T @ (q if b is None else b @ q))
        v = q @ y
    return theta, v


@pytest.mark.parametrize("eps", [0.0, 1e-7])
@pytest.mark.parametrize("case", ["generic", "pencil", "cluster_cut"])
def test_extraction_on_numpy_real_form_pairs(case, eps):
    sl = pytest.importorskip("scipy.linalg")
    n, lowest = 40, 4
    h, s = H.extraction_case(case, n, lowest)
    theta, v = real_pairs(h, s, lowest, eps)
    ref = sl.eigh(h, s, eigvals_only=True)
    second = None if s is None else H.dense_csr(s)
    lam, x = solver.hermitian_eigenpairs(theta, v, lowest, second)
    assert lam.shape == (lowest,) and x.shape == (n, lowest) and x.dtype == np.complex128
    # exact pairs: eigh's eigenvalues to 1e-12; perturbed ones are Ritz values, off by the square of their residual
    H.check_extraction(h, s, theta, v, lam, x, ref, tol_lambda=1e-12 if eps == 0.0 else None)
    if s is not None:          # the lower triangle of S gives the same numbers
        lam2, x2 = solver.hermitian_eigenpairs(theta, v, lowest, H.dense_csr(s, lower=True), lower=True)
        H.check_extraction(h, s, theta, v, lam2, x2, ref, tol_lambda=1e-12 if eps == 0.0 else None)


def test_the_cluster_cut_keeps_gram_eigenvalues_above_one():
    """the cut goes through a triple eigenvalue: the real span is no complex subspace, and still the kept eigenvalues of G are >= 1"""
    lowest = 4
    h, _ = H.extraction_case("cluster_cut", 40, lowest)
    _, v = real_pairs(h, None, lowest)
    z = v[0::2] + 1j * v[1::2]
    g = np.linalg.eigvalsh(z.conj().T @ z)
    assert np.all(g[lowest:] >= 1.0 - 1e-12) and np.allclose(g + g[::-1], 2.0, atol=1e-12)


# ---- the array extraction -----------------------------------------------------------------------------------------------------------
def test_scipy_and_torch_complex_input_is_handed_over_as_it_stands():
    indptr, indices, data = H.hermitian_csr(17, "random", False)
    rp, ci, vv = engine_c.hermitian_arrays(indptr, indices, data, 17)
    assert rp.dtype == np.int64 and ci.dtype == np.int32 and vv.dtype == np.complex128
    assert np.shares_memory(vv, data) and vv.size == data.size          # no copy, no expansion
    sp = pytest.importorskip("scipy.sparse")
    m = sp.csr_matrix((data, indices, indptr), shape=(17, 17))
    rp, ci, vv = engine_c.hermitian_arrays(m)
    assert np.shares_memory(vv, m.data) and np.array_equal(ci, m.indices) and vv.size == m.nnz
    import torch
    t = torch.sparse_csr_tensor(torch.tensor(indptr), torch.tensor(indices), torch.tensor(data), size=(17, 17))
    assert t.dtype == torch.complex128
    rp, ci, vv = engine_c.hermitian_arrays(t)
    assert vv.dtype == np.complex128 and vv.ctypes.data == t.values().data_ptr() and np.array_equal(vv, data)
    with pytest.raises(TypeError, match="complex128"):
        engine_c.hermitian_arrays(indptr, indices, data.real.copy(), 17)
    with pytest.raises(TypeError, match="complex128"):
        engine_c.hermitian_arrays(indptr, indices, data.astype(np.complex64), 17)


def test_the_python_checks_of_the_fortran_door():
    indptr, indices, data = H.hermitian_csr(17, "banded", False)
    engine_c.check_hermitian(indptr, indices, data, 17)
    rows = np.repeat(np.arange(17), np.diff(indptr))
    bad = data.copy()
    p = int(np.flatnonzero(rows == indices)[3])
    bad[p] = bad[p].real + 0.25j
    with pytest.raises(ValueError, match=rf"diagonal entry {p} \(row {rows[p]}\) has the imaginary part 0.25"):
        engine_c.check_hermitian(indptr, indices, bad, 17)
    bad[p] = complex(bad[p].real, -0.0)          # -0.0 is a real diagonal
    engine_c.check_hermitian(indptr, indices, bad, 17)
    with pytest.raises(ValueError, match="above the diagonal"):
        engine_c.check_hermitian(indptr, indices, data, 17, 0, True)
    with pytest.raises(ValueError, match="out of range"):
        engine_c.check_hermitian(indptr, indices + 1, data, 17)


def test_update_values_takes_complex_for_hermitian_operators_only():
    with pytest.raises(TypeError, match="expected complex128"):
        engine_c.update_values_array(np.ones(4), 4, pairs=True)
    with pytest.raises(TypeError, match="expected float64"):
        engine_c.update_values_array(np.ones(4, dtype=np.complex128), 4)
    z = np.arange(4) + 1j
    host, dev = engine_c.update_values_array(z, 4, pairs=True)
    assert dev is None and np.shares_memory(host, z)
    with pytest.raises(ValueError, match="saw 4 values"):
        engine_c.update_values_array(z[:3], 4, pairs=True)


def test_the_guess_of_a_complex_vector_is_two_real_ones():
    x = np.array([[1 + 2j], [3 - 1j]])
    g = solver._hermitian_guess(x, 2, 4)
    assert g.shape == (4, 2) and g[:, 0].tolist() == [1, 2, 3, -1] and g[:, 1].tolist() == [-2, 1, 1, 3]
    assert np.array_equal(g[:, 1], H.interleave(1j * x)[:, 0])
