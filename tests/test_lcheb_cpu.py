"""CPU: the Chebyshev-filtered correction with a Lanczos bound (method "LCHEB", code 5 with the degree in bits 8..15) without a GPU - the
code and the strings agree in every layer that carries them, the feature adds no entry point and leaves the ABI version alone, the Python
front ends refuse what the method does not serve before any engine call, and the numpy restatement of the bound (tests/lcheb_inputs.py)
never falls below the largest eigenvalue and reproduces the recorded iteration counts."""
import os
import re
import subprocess

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd import _abi, engine_c, solver
import cheb_inputs as CI
import lcheb_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fortran_davidson_amd", "csrc")
LIBDIR = os.path.join(ROOT, "fortran_davidson_amd", "lib")


def read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


# ---- 1. the code and the strings ----------------------------------------------------------------------------------------------------
def test_the_method_code_is_five_and_carries_the_degree_in_every_layer():
    hdr = read(ROOT, "include", "davidson_hip.h")
    assert re.search(r"enum\s*\{\s*DAV_METHOD_LCHEB\s*=\s*5\s*\};", hdr)
    assert hdr.index("DAV_METHOD_CHEB = 4") < hdr.index("DAV_METHOD_LCHEB = 5")
    assert re.search(r"#define DAV_METHOD_LCHEB_DEGREE\(d\) \(5 \| \(\(d\) << 8\)\)", hdr)
    assert re.search(r"#define DAV_HIP_ABI_VERSION 109\b", hdr) and engine_c.ABI_VERSION == 109
    assert '"LCHEB correction: "' in hdr and "agree to\n * rounding, not to bits" in hdr
    assert re.search(r"LANCZOS_STEPS = 12;", read(CSRC, "kernels.h")) and I.STEPS == 12
    # Python
    assert engine_c.METHOD_LCHEB == 5 and engine_c.method_lcheb() == 5 and engine_c.method_lcheb(16) == 5 + 16 * 256 == 4101
    assert solver._method_code("LCHEB") == 5 and solver._method_code("LCHEB16") == 5 + 16 * 256
    assert solver._method_code("LCHEB1") == 261 and solver._method_code("LCHEB64") == 5 | 64 << 8
    assert [solver._method_code(m) for m in ("DPR", "GJD", "BDPR", "CHEB", "CHEB16", "nonsense")] == [0, 1, 3, 4, 4100, 2]
    for bad in ("LCHEB0", "LCHEB65", "LCHEB-1", "LCHEBx", "LCHEB1.5", "LCHEB 4"):
        with pytest.raises(ValueError, match="1 <= d <= 64"):
            solver._method_code(bad)
    # (Fortran - the parameter, the parser, the DPR side of the loop, the names the doors carry the degree in: tests/test_methods_cpu.py,
    # through the compiled module)


def test_the_feature_adds_no_entry_point():
    def exported(lib, prefix):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        return {m.group(1) for m in re.finditer(rf"\s[TW]\s+({prefix}\w+)$", out, re.M)}
    product = exported(os.path.join(LIBDIR, "libdavidson_hip.so"), "dav_")
    test_build = exported(os.path.join(LIBDIR, "test", "libdavidson_hip.so"), "dav_")
    assert product == set(_abi.DAV) - set(_abi.TEST_BUILD_ONLY) and len(_abi.DAV) == 75 + 12
    assert test_build == set(_abi.DAV)
    doors = exported(os.path.join(LIBDIR, "libfortran_davidson_amd.so"), "fd_")
    assert doors == set(_abi.FD) and len(_abi.FD) == 41
    assert not any("cheb" in name.lower() or "lanczos" in name.lower() for name in product | test_build | doors)
    # ... and the kernels are in the library
    syms = subprocess.run(["strings", os.path.join(LIBDIR, "libdavidson_hip.so")], capture_output=True, text=True, check=True).stdout
    for kernel in ("lanczos_start_kernel", "lanczos_first_kernel", "lanczos_second_kernel", "lanczos_finish_kernel"):
        assert kernel in syms, kernel


# ---- 2. the front ends refuse before any engine call -------------------------------------------------------------------------------------
class _NoCalls:
    """a library stand-in whose every symbol fails the test when called"""
    def __getattr__(self, name):
        def call(*args):
            raise AssertionError(f"{name} was called")
        return call


def test_front_ends_refuse_before_any_engine_call(monkeypatch):
    monkeypatch.setattr(solver, "fortran_lib", lambda: _NoCalls())
    a = CI.laplacian2d(5, 1)
    rp, ci, vv = CI.csr_of(a)
    for method in ("LCHEB", "LCHEB16"):
        with pytest.raises(ValueError, match="LCHEB.*standard problems only"):
            solver.generalized_eigensolver(a, 2, method, 10, 1e-8, None, np.eye(25))
        with pytest.raises(ValueError, match="LCHEB.*host callbacks are not served"):
            solver.generalized_eigensolver_free(lambda x: a @ x, 25, 2, method, 10, 1e-8, 20, lambda x: x)
        with pytest.raises(ValueError, match="standard problems only"):
            solver.generalized_eigensolver_sparse(rp, ci, vv, 2, method, 10, 1e-8, second=(rp, ci, vv))
        with pytest.raises(ValueError, match="standard problems only"):
            solver.generalized_eigensolver_bsr(rp, ci, vv.reshape(-1, 1, 1), 2, method, 10, 1e-8, second=(rp, ci, vv.reshape(-1, 1, 1)))
    with pytest.raises(ValueError, match="1 <= d <= 64"):
        solver.generalized_eigensolver(a, 2, "LCHEB65", 10, 1e-8)
    with pytest.raises(ValueError, match="1 <= d <= 64"):
        solver.generalized_eigensolver_sparse(rp, ci, vv, 2, "LCHEB0", 10, 1e-8)
    check = solver._check_lcheb
    for other in ("DPR", "GJD", "BDPR", "CHEB", "CHEB12"):
        check(other, gev=True, host_callbacks=True)
    check("LCHEB")
    check("LCHEB33")
    with pytest.raises(ValueError, match="standard problems only"):
        check("LCHEB12", gev=True)

    class Eng(fd.DavidsonEngine):
        def __init__(self, gev):
            self.lib, self.gev, self.n, self.nranks, self.lowest, self.max_dim, self.p = _NoCalls(), gev, 25, 1, 2, 20, None
    with pytest.raises(ValueError, match="standard problems only"):
        Eng(True).solve("LCHEB")
    with pytest.raises(ValueError, match="1 <= d <= 64"):
        Eng(False).solve("LCHEB99")
    # a standard problem passes the check whatever kind A is: the first engine call is reached
    with pytest.raises(AssertionError, match="fd_engine_solve was called"):
        Eng(False).solve("LCHEB16")


# ---- 3. the restated bound --------------------------------------------------------------------------------------------------------------
def test_the_start_vector():
    u = I.start_vector(1000)
    assert (np.abs(u) < 1.0).all() and abs(u.mean()) < 0.1 and np.unique(u).size == 1000
    assert np.array_equal(I.start_vector(10), u[:10])                    # a function of the global row alone
    z = int(I.O._splitmix64(np.array([1], dtype=np.uint64))[0])
    assert u[0] == (z >> 11) * 2.0 ** -52 - 1.0


@pytest.mark.parametrize("name", sorted(I.bound_matrices()))
def test_the_restated_bound_is_never_below_the_largest_eigenvalue(name):
    a = I.bound_matrices()[name]
    top = np.linalg.eigvalsh(a).max()
    ratios = [I.lanczos_bound(a, k) / top for k in (4, 8, 12, 20)]
    print(f"{name}: bound / lambda_max at 4, 8, 12, 20 steps = {[round(float(r), 3) for r in ratios]}")
    assert min(ratios) >= 1.0, (name, ratios)
    assert max(ratios) <= 1.5, (name, ratios)                             # the largest Gershgorin row of a tridiagonal matrix: < 2 |T|


def test_the_rule_on_small_cases():
    trace = []
    assert I.lanczos_bound(np.zeros((5, 5)), trace=trace) == 0.0 and trace == [(0.0, 0.0)]         # stops at once: beta <= 0
    trace = []
    assert I.lanczos_bound(np.eye(7), trace=trace) == 1.0 and len(trace) == 1                       # A v = v: alpha = 1, beta = 0
    assert abs(I.lanczos_bound(np.array([[3.0]])) - 3.0) < 1e-15                                     # min(12, n) = 1 step
    a = np.diag([1.0, 2.0, 5.0])
    trace = []
    b = I.lanczos_bound(a, trace=trace)
    assert len(trace) == 3 and b >= 5.0                                                              # n steps: T is similar to A
    al, be = np.array(trace).T
    rows = al + np.concatenate([[0.0], be[:-1]]) + np.concatenate([be[:-1], [0.0]])
    assert b == rows.max() + be[-1]
    assert np.isnan(I.lanczos_bound(np.full((4, 4), np.nan)))


def test_the_first_coefficient_and_its_inverse():
    theta = np.array([4.0, 4.8, 6.0])
    b = 8.0 * (1 + 2.0 ** -30)
    c0 = I.first_coefficient(theta, 2, 1, b)
    ok, a0, lo, bb = CI.interval(theta, 2, 1, b)
    assert ok and lo == 4.8 and c0 == ((bb - lo) / 2 / (a0 - (lo + bb) / 2)) / ((bb - lo) / 2)
    r = np.random.default_rng(0).standard_normal((40, 2))
    assert I.coefficient_of_block(r, c0 * r) == float(c0)
    assert I.coefficient_of_block(r, c0 * r + 1e-13) is None
    found = I.bounds_giving(float(c0), theta, 2, 1, b * (1 + 40 * 2.0 ** -52))
    assert b in found and found.size <= 4 and found.max() - found.min() <= 4 * 2.0 ** -52 * b
    assert np.isnan(I.first_coefficient(theta, 2, 1, 3.0)) and np.isnan(I.first_coefficient(theta, 2, 1, np.inf))


def test_the_stencils_blocks_are_rank_deficient_and_the_others_are_not():
    """Why the engine's iteration counts on the stencil are not the restatement's (tests/test_lcheb_gpu.py): its start
    vectors are unit vectors at one end of a band of five diagonals, a polynomial of degree 10 reaches 20 rows further, so m corrections
    live in fewer than 2 m rows from the second iteration on.  What fills the dependent columns decides the next basis: the oracle's
    Householder QR here, unit vectors at the next entries of the start order in the engine."""
    for name in ("stencil300_l4", "stencil300_l8"):
        a, lowest = I.table_inputs()[name]
        ranks = I.block_ranks(a, lowest)
        assert any(rank < cols for cols, rank in ranks[1:]), (name, ranks)
    for name in ("noisy_lap16_l4", "lap24_l8", "block240_b4"):
        a, lowest = I.table_inputs()[name]
        ranks = I.block_ranks(a, lowest)
        assert all(rank == cols for cols, rank in ranks), (name, ranks)


# ---- the recorded iteration counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(I.TABLE))
def test_the_restatement_reproduces_the_recorded_iteration_counts(name):
    """the three LCHEB columns of every row; scalar DPR's column where its hundreds of iterations take about a second (the other rows'
    were recorded by the same call)"""
    a, lowest = I.table_inputs()[name]
    ref = np.linalg.eigvalsh(a)[:lowest]
    dpr, d6, d10, d16 = I.TABLE[name]
    for method, want in (("LCHEB6", d6), ("LCHEB10", d10), ("LCHEB16", d16)):
        lam, vec, it = I.restated_solve(a, lowest, method)
        assert it == want, (name, method, it)
        assert np.abs(lam - ref).max() < 1e-8 and np.linalg.norm(a @ vec - vec * lam[None, :], axis=0).max() < 1e-8
    if name in ("noisy_lap16_l4", "block240_b4"):
        assert I.restated_solve(a, lowest, "DPR")[2] == dpr
    assert 3 * d10 <= dpr and 3 * d16 <= dpr and d16 <= d10 <= d6
    assert I.restated_solve(a, lowest, "LCHEB")[2] == d10
