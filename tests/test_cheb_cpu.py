"""CPU: the Chebyshev-filtered correction (method "CHEB", code 4 with the degree in bits 8..15) without a GPU - the code and the degree
encoding exist and agree in every layer that carries them, the feature adds no entry point, the Python front ends refuse what the method
does not serve before any engine call, and the numpy restatement (tests/cheb_inputs.py) satisfies the filter identity, converges and
reproduces the recorded iteration counts of scalar DPR and of CHEB at three degrees under two policies."""
import os
import re
import subprocess

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd import _abi, engine_c, solver
import bdpr_inputs as BI
import cheb_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fortran_davidson_amd", "csrc")
LIBDIR = os.path.join(ROOT, "fortran_davidson_amd", "lib")


def read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_the_method_code_is_four_and_carries_the_degree_in_every_layer():
    hdr = read(ROOT, "include", "davidson_hip.h")
    assert re.search(r"enum\s*\{\s*DAV_METHOD_CHEB\s*=\s*4\s*\};", hdr)
    assert re.search(r"#define DAV_METHOD_CHEB_DEGREE\(d\) \(4 \| \(\(d\) << 8\)\)", hdr)
    assert re.search(r"#define DAV_HIP_ABI_VERSION 109\b", hdr)
    kern = read(CSRC, "kernels.h")
    assert re.search(r"CHEB_MAX_DEGREE = 64;", kern) and re.search(r"CHEB_DEFAULT_DEGREE = 10;", kern)
    assert I.DEFAULT_DEGREE == 10
    # (the engine splits the code before it compares it: tests/test_exact_phases_gpu.py compares the codes with and without a degree)
    # Python
    assert engine_c.METHOD_CHEB == 4 and engine_c.method_cheb() == 4 and engine_c.method_cheb(16) == 4 | 16 << 8 == 4100
    assert solver._method_code("CHEB") == 4 and solver._method_code("CHEB1") == 260 and solver._method_code("CHEB64") == 4 | 64 << 8
    assert [solver._method_code(m) for m in ("DPR", "GJD", "BDPR", "nonsense")] == [0, 1, 3, 2]
    for bad in ("CHEB0", "CHEB65", "CHEB-1", "CHEBx", "CHEB1.5", "CHEB 4"):
        with pytest.raises(ValueError, match="1 <= d <= 64"):
            solver._method_code(bad)
    # (Fortran - the parameter, the driver's parser and its message, the DPR side of the loop, the names the doors carry the degree in:
    # tests/test_methods_cpu.py, through the compiled module)


def test_the_feature_adds_no_entry_point():
    def exported(lib, prefix):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        return {m.group(1) for m in re.finditer(rf"\s[TW]\s+({prefix}\w+)$", out, re.M)}
    product = exported(os.path.join(LIBDIR, "libdavidson_hip.so"), "dav_")
    test_build = exported(os.path.join(LIBDIR, "test", "libdavidson_hip.so"), "dav_")
    assert product == set(_abi.DAV) - set(_abi.TEST_BUILD_ONLY)
    assert test_build == set(_abi.DAV)
    doors = exported(os.path.join(LIBDIR, "libfortran_davidson_amd.so"), "fd_")
    assert doors == set(_abi.FD)
    assert not any("cheb" in name.lower() for name in product | test_build | doors)
    # ... and the kernels are in the library
    syms = subprocess.run(["strings", os.path.join(LIBDIR, "libdavidson_hip.so")], capture_output=True, text=True, check=True).stdout
    for kernel in ("cheb_row_bound_kernel", "cheb_coef_kernel", "cheb_step_kernel"):
        assert kernel in syms, kernel


class _NoCalls:
    """a library stand-in whose every symbol fails the test when called"""
    def __getattr__(self, name):
        def call(*args):
            raise AssertionError(f"{name} was called")
        return call


def test_front_ends_refuse_before_any_engine_call(monkeypatch):
    monkeypatch.setattr(solver, "fortran_lib", lambda: _NoCalls())
    a = I.laplacian2d(5, 1)
    rp, ci, vv = I.csr_of(a)
    for method in ("CHEB", "CHEB16"):
        with pytest.raises(ValueError, match="CHEB.*CSR or BSR"):
            solver.generalized_eigensolver(a, 2, method, 10, 1e-8)
        with pytest.raises(ValueError, match="CHEB.*CSR or BSR"):
            solver.generalized_eigensolver_free(lambda x: a @ x, 25, 2, method, 10, 1e-8, 20, lambda x: x)
        with pytest.raises(ValueError, match="standard problems only"):
            solver.generalized_eigensolver_sparse(rp, ci, vv, 2, method, 10, 1e-8, second=(rp, ci, vv))
        with pytest.raises(ValueError, match="standard problems only"):
            solver.generalized_eigensolver_bsr(rp, ci, vv.reshape(-1, 1, 1), 2, method, 10, 1e-8, second=(rp, ci, vv.reshape(-1, 1, 1)))
    with pytest.raises(ValueError, match="1 <= d <= 64"):
        solver.generalized_eigensolver_sparse(rp, ci, vv, 2, "CHEB65", 10, 1e-8)
    with pytest.raises(ValueError, match="1 <= d <= 64"):
        solver.generalized_eigensolver_bsr(rp, ci, vv.reshape(-1, 1, 1), 2, "CHEB0", 10, 1e-8)
    # the resident engine: what its operators are is known from the set calls
    check = solver._check_cheb
    check("DPR", False)
    check("GJD", False, gev=True)
    check("BDPR", False)
    check("CHEB", True)
    check("CHEB33", True)
    with pytest.raises(ValueError, match="operator A in CSR or BSR form"):
        check("CHEB", False)
    with pytest.raises(ValueError, match="standard problems only"):
        check("CHEB12", True, gev=True)

    class Eng(fd.DavidsonEngine):
        def __init__(self):
            self.lib, self.gev, self.n, self.nranks = _NoCalls(), False, 25, 1
    eng = Eng()
    with pytest.raises(ValueError, match="operator A in CSR or BSR form"):
        eng.solve("CHEB")
    eng._note_blocks(1, None, sparse=True)
    eng._note_blocks(1, None)                        # another set call: no longer sparse
    with pytest.raises(ValueError, match="operator A in CSR or BSR form"):
        eng.solve("CHEB8")
    eng._note_blocks(1, 4)
    eng.gev = True
    with pytest.raises(ValueError, match="standard problems only"):
        eng.solve("CHEB")


@pytest.mark.parametrize("degree", [1, 2, 3, 12, 25])
def test_the_recurrence_is_the_filter_minus_its_value_at_theta(degree):
    """z_d = p_d(A) x - p_d(theta) x for real Ritz pairs, in long double against a direct evaluation of the filter"""
    a = I.laplacian2d(12, 3)
    n, m, lowest = a.shape[0], 9, 4
    v = np.linalg.qr(np.random.default_rng(5).standard_normal((n, m)))[0]
    theta, y = np.linalg.eigh(v.T @ a @ v)
    x = (v @ y).astype(np.longdouble)
    r = I.Product(a)(x) - x * theta[None, :].astype(np.longdouble)
    for ncorr in (m, lowest):
        z = I.cheb_correction(a, theta, r, ncorr, lowest, degree, dtype=np.longdouble)
        direct = I.filter_direct(a, theta, x, ncorr, lowest, degree)
        scale = np.abs(direct).max()
        assert scale > 0 and float(np.abs(z - direct).max() / scale) < 1e-15, (degree, ncorr)
    z64 = I.cheb_correction(a, theta, r.astype(np.float64), m, lowest, degree)
    assert float(np.abs(z64 - direct_all(a, theta, x, m, lowest, degree)).max() / scale) < 1e-12


def direct_all(a, theta, x, m, lowest, degree):
    return I.filter_direct(a, theta, x, m, lowest, degree)


def test_the_interval_rule():
    theta = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    ok, a0, a, b = I.interval(theta, 6, 2, 65.0)             # the reference policy: theta_{min(6, 4) - 1} = 4 > theta_1 + delta = 3
    assert ok and (a0, a, b) == (1.0, 4.0, 65.0)
    ok, a0, a, b = I.interval(theta, 2, 2, 65.0)             # ncorr = lowest: the last wanted value stays outside the damped interval
    assert ok and (a0, a, b) == (1.0, 3.0, 65.0)
    ok, a0, a, b = I.interval(theta, 6, 3, 6.0625)           # clipped below the bound
    assert ok and a == 6.0625 - 5.0625 / 64 < 6.0
    assert not I.interval(theta, 6, 2, 1.0)[0] and not I.interval(theta, 6, 2, 0.5)[0]          # b > a0 does not hold
    assert not I.interval(theta, 6, 2, np.inf)[0] and not I.interval(theta, 6, 2, np.nan)[0]
    assert not I.interval(np.array([1.0, np.nan]), 2, 1, 9.0)[0]
    assert not I.cheb_correction(np.zeros((4, 4)), np.zeros(2), np.ones((4, 2)), 2, 1, 5).any()     # a zero matrix: a zero block
    assert I.row_bound(np.array([[1.0, -2.0], [-2.0, 0.5]])) == 3.0 and I.row_bound(np.zeros((3, 3))) == 0.0


@pytest.mark.parametrize("name", sorted(I.TABLE))
def test_the_restatement_converges_and_reproduces_the_recorded_iteration_counts(name):
    a, lowest = I.table_inputs()[name]
    ref = np.linalg.eigvalsh(a)[:lowest]
    for policy in ("all", "unconverged"):
        got = []
        for method in ("DPR", "CHEB6", "CHEB10", "CHEB16"):
            lam, vec, it = I.restated_solve(a, lowest, method, policy)
            got.append(it)
            if method != "DPR":
                assert it <= I.MAX_ITERATIONS, (name, policy, method)
                assert np.abs(lam - ref).max() < 1e-8, (name, policy, method)
                assert np.linalg.norm(a @ vec - vec * lam[None, :], axis=0).max() < 1e-8, (name, policy, method)
        assert tuple(got) == I.TABLE[name][policy], (name, policy, got)
        dpr, _, d10, d16 = got
        assert 3 * d10 <= dpr and 3 * d16 <= dpr, (name, policy, got)
    assert np.array_equal(I.restated_solve(a, lowest, "CHEB", "all")[0], I.restated_solve(a, lowest, "CHEB10", "all")[0])
