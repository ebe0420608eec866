"""CPU: the block-diagonal preconditioned correction (method "BDPR", code 3) without a GPU - the code exists and agrees in every layer
that carries it, the feature adds no entry point, the numpy restatement of the solve (tests/bdpr_inputs.py) reproduces the recorded
iteration counts of scalar and block DPR, and the Python front ends refuse what the method does not serve before any engine call."""
import os
import re
import subprocess

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd import _abi, engine_c, solver
import bdpr_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fortran_davidson_amd", "lib")


def read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_the_method_code_is_three_in_every_layer():
    hdr = read(ROOT, "include", "davidson_hip.h")
    enum = re.search(r"enum\s*\{\s*DAV_METHOD_DPR\s*=\s*0.*?\};", hdr, re.S).group(0)
    enum = re.sub(r"/\*.*?\*/", "", enum, flags=re.S)
    codes = {k: int(v) for k, v in re.findall(r"(DAV_METHOD_\w+)\s*=\s*(\d+)", enum)}
    assert codes == {"DAV_METHOD_DPR": 0, "DAV_METHOD_GJD": 1, "DAV_METHOD_NONE": 2, "DAV_METHOD_BDPR": 3}
    assert re.search(r"#define DAV_HIP_ABI_VERSION 109\b", hdr)
    assert (engine_c.METHOD_DPR, engine_c.METHOD_GJD, engine_c.METHOD_BDPR) == (0, 1, 3)
    assert solver._METHOD == {"DPR": 0, "GJD": 1, "BDPR": 3}
    # (the Fortran parameters, the driver's parser, the names the doors hand it - 0: "DPR", 1: "GJD", 2: "XXX", 3: "BDPR" - and the
    # driver's "(DPR, GJD or BDPR)" message: tests/test_methods_cpu.py, through the compiled module)


def test_the_feature_adds_no_entry_point():
    """every dav_* / fd_* symbol the libraries export is one the headers (through _abi, which tests/test_abi_cpu.py holds equal to them
    name for name) already declare"""
    def exported(lib, prefix):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        return {m.group(1) for m in re.finditer(rf"\s[TW]\s+({prefix}\w+)$", out, re.M)}
    product = exported(os.path.join(LIBDIR, "libdavidson_hip.so"), "dav_")
    test_build = exported(os.path.join(LIBDIR, "test", "libdavidson_hip.so"), "dav_")
    assert product == set(_abi.DAV) - set(_abi.TEST_BUILD_ONLY)
    assert test_build == set(_abi.DAV)
    doors = exported(os.path.join(LIBDIR, "libfortran_davidson_amd.so"), "fd_")
    assert doors == set(_abi.FD)
    assert not any("bdpr" in name.lower() for name in product | test_build | doors)


@pytest.mark.parametrize("case", sorted(I.TABLE), ids=lambda c: f"n{c[0]}_b{c[1]}_{'gev' if c[2] else 'std'}_seed{c[3]}")
def test_the_restatement_reproduces_the_recorded_iteration_counts(case):
    n, b, gev, seed = case
    a, bm = I.block_matrix(n, b, seed, gev)
    if gev:
        # B = L L^T: the eigenvalues of L^-1 A L^-T
        l = np.linalg.cholesky(bm)
        ref = np.linalg.eigvalsh(np.linalg.solve(l, np.linalg.solve(l, a).T))[:4]
    else:
        ref = np.linalg.eigvalsh(a)[:4]
    got = []
    for method in ("DPR", "BDPR"):
        lam, vec, it = I.restated_solve(a, bm, b, 4, method)
        assert np.abs(lam - ref).max() < 1e-8, (case, method)
        res = a @ vec - (bm @ vec if gev else vec) * lam[None, :]
        assert np.linalg.norm(res, axis=0).max() < 1e-8, (case, method)
        got.append(it)
    assert tuple(got) == I.TABLE[case]


def test_the_elimination_follows_the_pivot_rule():
    rng = np.random.default_rng(0)
    for b in (1, 2, 3, 5, 8, 16):
        m = rng.standard_normal((40, b, b))
        r = rng.standard_normal((40, b))
        t, rho, singular = I.eliminate_batch(m, r)
        assert not singular.any() and (rho >= 1.0).all()
        assert np.abs(np.einsum("sij,sj->si", m, t) - r).max() < 1e-9
        assert np.abs(t - np.linalg.solve(m, r[:, :, None])[:, :, 0]).max() < 1e-8
    # equal candidates: the lowest row is the pivot, and the second pivot of [[1, 1], [1, 1]] is exactly zero
    t, rho = I.eliminate(np.ones((2, 2)), np.array([1.0, 2.0]))
    assert not t.any() and not np.signbit(t).any()
    t, rho = I.eliminate(np.zeros((3, 3)), np.ones(3))
    assert not t.any() and rho == 1.0
    t, _ = I.eliminate(np.array([[2.0, 1.0], [-2.0, 1.0]]), np.array([3.0, -1.0]))      # |2| = |-2|: row 0 first
    assert np.array_equal(t, [1.0, 1.0])
    # a matrix whose elimination grows: rho says so
    w = np.tril(-np.ones((6, 6)), -1) + np.eye(6)
    w[:, -1] = 1.0
    _, rho = I.eliminate(w, np.ones(6))
    assert rho == 2.0 ** 5


def test_bsr_arrays_of_the_inputs():
    a, _ = I.block_matrix(48, 4, 5)
    for lower in (False, True):
        for split in (None, 3):
            rp, ci, vv = I.bsr_of(a, 4, lower=lower, split=split)
            dense = np.zeros_like(a)
            for row in range(12):
                for p in range(rp[row], rp[row + 1]):
                    dense[row*4:(row+1)*4, ci[p]*4:(ci[p]+1)*4] += vv[p]
            want = a
            if lower:
                keep = np.kron(np.tril(np.ones((12, 12))), np.ones((4, 4)))
                want = a * keep
            assert np.abs(dense - want).max() < 1e-15
            d = I.diagonal_blocks(rp, ci, vv)
            assert np.abs(d - np.stack([a[i*4:(i+1)*4, i*4:(i+1)*4] for i in range(12)])).max() < 1e-15
            if split is not None:
                assert (np.bincount(ci[np.repeat(np.arange(12), np.diff(rp)) == ci], minlength=12)[::2] == 2).all()


class _NoCalls:
    """a library stand-in whose every symbol fails the test when called"""
    def __getattr__(self, name):
        def call(*args):
            raise AssertionError(f"{name} was called")
        return call


def test_front_ends_refuse_before_any_engine_call(monkeypatch):
    monkeypatch.setattr(solver, "fortran_lib", lambda: _NoCalls())
    a, bm = I.block_matrix(24, 4, 1, gev=True)
    rp, ci, vv = I.bsr_of(a, 4)
    with pytest.raises(ValueError, match="BDPR.*BSR"):
        solver.generalized_eigensolver(a, 2, "BDPR", 10, 1e-8)
    with pytest.raises(ValueError, match="BDPR.*BSR"):
        solver.generalized_eigensolver_sparse(np.arange(25), np.arange(24), np.ones(24), 2, "BDPR", 10, 1e-8)
    # a B of another block size, values that are not float64, a data array that is not (nnzb, b, b)
    rp2, ci2, vv2 = I.bsr_of(bm, 2)
    with pytest.raises(ValueError, match="block size"):
        solver.generalized_eigensolver_bsr(rp, ci, vv, 2, "BDPR", 10, 1e-8, second=(rp2, ci2, vv2))
    with pytest.raises(ValueError, match=r"shape \(nnzb, b, b\)"):
        solver.generalized_eigensolver_bsr(rp, ci, vv.reshape(-1, 16), 2, "BDPR", 10, 1e-8)
    with pytest.raises(ValueError, match="multiple of the block size"):
        solver.generalized_eigensolver_bsr(rp, ci, vv, 2, "BDPR", 10, 1e-8, n=26)
    with pytest.raises(TypeError, match="float64"):
        solver.generalized_eigensolver_bsr(rp, ci, vv, 2, "BDPR", 10, 1e-8, initial_vectors=np.ones((24, 2), dtype=np.float32))
    with pytest.raises(ValueError):
        solver.generalized_eigensolver_bsr(rp, ci, vv, 2, "BDPR", 10, 1e-8, initial_vectors=np.ones((23, 2)))
    # the resident engine: what its operators are is known from the set calls
    check = solver._check_bdpr
    check("DPR", (None, None))
    check("GJD", (None, 4), gev=True)
    check("BDPR", (4, None))
    check("BDPR", (4, 4), gev=True)
    check("BDPR", (5, None), n=240, nranks=3)              # 80 rows per rank
    with pytest.raises(ValueError, match="operator A in BSR form"):
        check("BDPR", (None, None))
    with pytest.raises(ValueError, match="operator B in BSR form"):
        check("BDPR", (4, None), gev=True)
    with pytest.raises(ValueError, match="block size 2"):
        check("BDPR", (4, 2), gev=True)
    with pytest.raises(ValueError, match="divides the 80 rows"):
        check("BDPR", (3, None), n=240, nranks=3)
    assert callable(fd.DavidsonEngine.solve) and engine_c.CEngine.ritz_residual_correction.__defaults__ == (engine_c.METHOD_DPR,)
