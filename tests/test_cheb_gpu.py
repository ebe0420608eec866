"""GPU: the Chebyshev-filtered correction (method "CHEB", DAV_METHOD_CHEB; kernels in fortran_davidson_amd/csrc/k_cheb.hip and the fused
step of k_spmm.hip).  The correction block against the numpy restatement in long double; the fused step against the separate one bit for
bit; new values on a kept pattern; the refusals and the degenerate interval; three ranks against one; solves against eigvalsh and against
scalar DPR's iteration counts; policies, device-side Rayleigh-Ritz, warm start; the one-call front ends and a Fortran program."""
import os
import re

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import (METHOD_CHEB, METHOD_DPR, OP_A, OP_B, PANEL_R, PANEL_V, PANEL_W, DavidsonHipError,
                                           method_cheb)
import bdpr_inputs as BI
import cheb_inputs as I
from test_bdpr_gpu import PadRows, bits, set_bsr, three_ranks

pytestmark = pytest.mark.gpu
U = I.U
METHOD_NONE = 2
MS = (1, 5, 16, 17, 33)
DEGREES = (1, 2, 3, 10, 25)


# ---- inputs, computed once ---------------------------------------------------------------------------------------------------------------
def sparse_matrix(n, seed):
    """about seven entries per row, a nearly flat diagonal, both signs"""
    return I.random_sparse(n, 6.0 / n, seed, grade=0.5 / n)


def long_row_matrix():
    """n = 1100: row (and column) 0 holds 1099 entries - more than one chunk of the CSR product (1024) -, row 5 is empty, the rest is a
    band of both signs"""
    n = 1100
    rng = np.random.default_rng(11)
    a = np.zeros((n, n))
    i = np.arange(n - 1)
    a[i, i + 1] = a[i + 1, i] = -0.5
    i = np.arange(n - 7)
    a[i, i + 7] = a[i + 7, i] = 0.25
    a[np.arange(n), np.arange(n)] = 2.0 + 0.001 * np.arange(n)
    a[0, 1:] = a[1:, 0] = 0.02 * rng.standard_normal(n - 1)
    a[5, :] = 0.0
    a[:, 5] = 0.0
    return a


_ritz_cache = {}


def ritz_pairs(key, a, m, seed):
    """real Ritz pairs of a random orthonormal basis: (V, W = A V, Y, theta)"""
    if (key, m) not in _ritz_cache:
        v = np.linalg.qr(np.random.default_rng(seed).standard_normal((a.shape[0], m)))[0]
        w = a @ v
        theta, y = np.linalg.eigh(v.T @ w)
        _ritz_cache[(key, m)] = (np.asfortranarray(v), np.asfortranarray(w), np.asfortranarray(y), theta)
    return _ritz_cache[(key, m)]


def correction(e, v, w, y, theta, lowest, method):
    """the Ritz phase on the panels V, W with the eigenpairs (theta, Y): ncorr = m.  Returns (R, T)"""
    m = v.shape[1]
    e.panel_put(PANEL_V, 0, v)
    e.panel_put(PANEL_W, 0, w)
    e.ritz_residual_correction(m, lowest, y, theta, method)
    return e.panel_get(PANEL_R, 0, m), e.panel_get(PANEL_V, m, m)


def check_block(a, prod, bound, r, t, theta, m, lowest, degree, where):
    """per column max |T - T_ld| <= 8 max(err_f64, d u) max |T_ld|: T_ld the restatement in long double from the R the engine wrote,
    err_f64 the relative error of the same restatement in float64.  Returns the largest ratio to the bar."""
    t_ld = I.cheb_correction(a, theta, r, m, lowest, degree, bound, np.longdouble, prod)
    t_64 = I.cheb_correction(a, theta, r, m, lowest, degree, bound)
    scale = np.abs(t_ld).max(axis=0)
    assert (scale > 0).all(), where
    err64 = (np.abs(t_64 - t_ld).max(axis=0) / scale).astype(np.float64)
    err = (np.abs(t - t_ld).max(axis=0) / scale).astype(np.float64)
    bar = 8.0 * np.maximum(err64, degree * U)
    ratio = float((err / bar).max())
    assert ratio <= 1.0, (where, ratio, err.max(), err64.max())
    return ratio


def run_cases(e, pads, key, a, lowest_of=lambda m: min(4, m), ms=MS, degrees=DEGREES, check=True):
    """every (m, degree) on the operator A the engine holds: the checks of test 1; returns {(m, degree): T} and the largest ratio"""
    prod, bound = I.Product(a), I.row_bound(a)
    out, worst = {}, 0.0
    for m in ms:
        v, w, y, theta = ritz_pairs(key, a, m, 1000 + m)
        lowest = lowest_of(m)
        r0, _ = correction(e, v, w, y, theta, lowest, METHOD_NONE)
        for degree in degrees:
            if pads is not None:
                pads.dirty(m, m)
            r, t = correction(e, v, w, y, theta, lowest, method_cheb(degree))
            out[(m, degree)] = t
            if not check:
                continue
            where = (key, m, degree)
            assert np.array_equal(bits(r), bits(r0)), where                      # R as the residual product wrote it
            assert np.array_equal(bits(e.panel_get(PANEL_V, 0, m)), bits(v)), where
            assert np.allclose(r, w @ y - (v @ y) * theta[None, :], rtol=0, atol=1e-12), where
            worst = max(worst, check_block(a, prod, bound, r, t, theta, m, lowest, degree, where))
            if pads is not None:
                assert not bits(pads.read(m, m)).any(), (where, "pad rows of the written columns are not +0.0")
    return out, worst


# ---- 1. the correction block against the restatement in long double -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [50, 301, 777])
def test_csr_block_matches_the_restatement(n):
    a = sparse_matrix(n, n)
    with fd.CEngine(n=n, max_cols=66) as e:
        pads = PadRows(e, n)
        for lower in (False, True):
            e.set_operator_csr(OP_A, *I.csr_of(a, lower), lower=lower)
            _, worst = run_cases(e, pads, ("csr", n), a)
            print(f"CSR n={n} lower={lower}: largest error / bar = {worst:.3f}")


@pytest.mark.parametrize("b", [1, 3, 16])
def test_bsr_block_matches_the_restatement(b):
    n = b * -(-300 // b)
    a, _ = BI.block_matrix(n, b, 20 + b)
    with fd.CEngine(n=n, max_cols=66) as e:
        pads = PadRows(e, n)
        for lower in (False, True):
            set_bsr(e, OP_A, BI.bsr_of(a, b, lower=lower), lower)
            _, worst = run_cases(e, pads, ("bsr", b), a)
            print(f"BSR b={b} lower={lower}: largest error / bar = {worst:.3f}")


def test_long_row_empty_row_and_negative_entries():
    a = long_row_matrix()
    n = a.shape[0]
    assert (a < 0).any() and not a[5].any() and np.count_nonzero(a[0]) > 1024
    with fd.CEngine(n=n, max_cols=66) as e:
        pads = PadRows(e, n)
        e.set_operator_csr(OP_A, *I.csr_of(a))
        out, worst = run_cases(e, pads, "long", a)
        print(f"CSR long row: largest error / bar = {worst:.3f}")
    for (m, degree), t in out.items():
        if degree > 1:
            assert t[0].all() and t[5].all()         # (the empty row still takes -c z + pi r)


# ---- 2. the fused step equals the separate one bit for bit --------------------------------------------------------------------------------
def test_fused_and_separate_step_agree_bit_for_bit(monkeypatch):
    """the CSR cases of test 1 - every degree, full and lower input, the long-row matrix - on engines created with DAV_CHEB_FUSE=0 and =1.
    That the knob was read shows in the statistics: the same applies, and the fused ones account the bytes their epilogue reads at the
    rows it writes - z and r in the first step of a correction, z, r and z_{k-1} in the later ones."""
    mats = {("csr", n): sparse_matrix(n, n) for n in (50, 301, 777)}
    mats["long"] = long_row_matrix()
    ms = (1, 16, 17, 33)
    got, traffic = {}, {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("DAV_CHEB_FUSE", fuse)
        for key, a in mats.items():
            with fd.CEngine(n=a.shape[0], max_cols=66) as e:
                for lower in (False, True):
                    e.set_operator_csr(OP_A, *I.csr_of(a, lower), lower=lower)
                    e.reset_stats()
                    got[(fuse, key, lower)] = run_cases(e, None, key, a, ms=ms, degrees=DEGREES, check=False)[0]
                    st = e.stats()
                    traffic[(fuse, key, lower)] = (st.applies, st.apply_cols, st.apply_bytes)
    for key, a in mats.items():
        for lower in (False, True):
            for case, t in got[("1", key, lower)].items():
                assert np.isfinite(t).all() and t.any()
                assert np.array_equal(bits(t), bits(got[("0", key, lower)][case])), (key, lower, case)
            separate, fused = traffic[("0", key, lower)], traffic[("1", key, lower)]
            assert separate[:2] == fused[:2] == (len(ms) * sum(d - 1 for d in DEGREES), sum(ms) * sum(d - 1 for d in DEGREES))
            extra = 8.0 * a.shape[0] * sum(ms) * sum(2 + 3 * (d - 2) for d in DEGREES if d >= 2)
            assert fused[2] - separate[2] == extra, (key, lower, fused, separate, extra)


# ---- 3. new values on a kept pattern --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["csr", "bsr"])
def test_new_values_reach_the_bound_and_the_block(kind):
    b, m, degree = 4, 16, 10
    n = 300
    if kind == "csr":
        a1 = sparse_matrix(n, 1)
        a2 = np.where(a1 != 0.0, 1.75 * a1, 0.0) + np.diag(0.3 * np.cos(np.arange(n)))      # same pattern, another bound
        arr1, arr2 = I.csr_of(a1), I.csr_of(a2)
        put = lambda e, arr: e.set_operator_csr(OP_A, *arr)                                 # noqa: E731
    else:
        a1, a2 = BI.block_matrix(n, b, 1)[0], 1.5 * BI.block_matrix(n, b, 2)[0]
        arr1, arr2 = BI.bsr_of(a1, b), BI.bsr_of(a2, b)
        put = lambda e, arr: set_bsr(e, OP_A, arr)                                          # noqa: E731
    assert np.array_equal(arr1[0], arr2[0]) and np.array_equal(arr1[1], arr2[1]) and I.row_bound(a1) != I.row_bound(a2)
    v, w, y, theta = ritz_pairs(("refresh", kind), a2, m, 5)
    with fd.CEngine(n=n, max_cols=2 * m) as e:
        e.keep_value_map(OP_A)
        put(e, arr1)
        _, t1 = correction(e, v, w, y, theta, 4, method_cheb(degree))
        e.update_operator_values(OP_A, arr2[2])
        _, t2 = correction(e, v, w, y, theta, 4, method_cheb(degree))
    with fd.CEngine(n=n, max_cols=2 * m) as e:
        put(e, arr2)
        _, fresh = correction(e, v, w, y, theta, 4, method_cheb(degree))
    assert not np.array_equal(bits(t1), bits(t2))
    assert np.array_equal(bits(t2), bits(fresh))


# ---- 4. refusals and the degenerate interval -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["generalized", "a_dense", "a_host", "degree_65"])
def test_what_the_method_does_not_serve_is_refused(case):
    n, m = 240, 5
    a = sparse_matrix(n, 3)
    v, w, y, theta = ritz_pairs("refuse", a, m, 4)
    method = METHOD_CHEB
    with fd.CEngine(n=n, max_cols=16, gev=case == "generalized") as e:
        if case == "generalized":
            e.set_operator_csr(OP_A, *I.csr_of(a))
            e.set_operator_csr(OP_B, *I.csr_of(np.eye(n)))
            want = "generalized problem"
        elif case == "a_dense":
            e.set_dense_host(OP_A, np.asfortranarray(a))
            want = "operator A is a dense matrix"
        elif case == "a_host":
            e.set_operator_host(OP_A, np.diag(a).copy())
            want = "operator A is a host callback"
        else:
            e.set_operator_csr(OP_A, *I.csr_of(a))
            method, want = method_cheb(65), "degree 65 is outside 1..64"
        mark = np.full((n, m), 3.25)
        e.panel_put(PANEL_V, m, mark)
        e.panel_put(PANEL_R, 0, mark)
        e.panel_put(PANEL_V, 0, v)
        e.panel_put(PANEL_W, 0, w)
        with pytest.raises(DavidsonHipError, match=re.escape(want)) as exc:
            e.ritz_residual_correction(m, 4, y, theta, method)
        assert "CHEB" in str(exc.value)
        assert np.array_equal(bits(e.panel_get(PANEL_V, 0, m)), bits(v)) and np.array_equal(bits(e.panel_get(PANEL_W, 0, m)), bits(w))
        assert np.array_equal(e.panel_get(PANEL_V, m, m), mark) and np.array_equal(e.panel_get(PANEL_R, 0, m), mark)
        if case in ("a_dense", "degree_65"):
            # the engine stays usable: scalar DPR on the same panels
            _, t = correction(e, v, w, y, theta, 4, METHOD_DPR)
            assert np.isfinite(t).all()


def test_a_zero_matrix_gives_a_zero_block():
    n, m = 300, 5
    rp = np.arange(n + 1, dtype=np.int64)
    v = np.asfortranarray(np.linalg.qr(np.random.default_rng(0).standard_normal((n, m)))[0])
    w = np.zeros((n, m), order="F")
    with fd.CEngine(n=n, max_cols=16) as e:
        pads = PadRows(e, n)
        e.set_operator_csr(OP_A, rp, np.arange(n, dtype=np.int32), np.zeros(n))      # stored zeros: b = 0 = a0
        e.panel_put(PANEL_V, m, np.full((n, m), 3.25))
        pads.dirty(m, m)
        r, t = correction(e, v, w, np.eye(m), np.zeros(m), 4, METHOD_CHEB)
        assert not bits(t).any() and not bits(pads.read(m, m)).any()                 # +0.0, not -0.0
        assert not r.any()


# ---- 5. three ranks against one ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["csr", "bsr"])
def test_three_ranks_match_one_rank(kind):
    m, degree = 17, 10
    if kind == "csr":
        n = 301                                           # 112 rows on ranks 0 and 1, 77 on rank 2
        a = sparse_matrix(n, 2)
        put = lambda e: e.set_operator_csr(OP_A, *I.csr_of(a))                              # noqa: E731
    else:
        n, b = 300, 3                                     # 112 is no multiple of 3: a block row straddles two ranks
        a, _ = BI.block_matrix(n, b, 4)
        put = lambda e: set_bsr(e, OP_A, BI.bsr_of(a, b))                                   # noqa: E731
    v, w, y, theta = ritz_pairs(("ranks", kind), a, m, 6)
    with fd.CEngine(n=n, max_cols=2 * m) as e:
        put(e)
        r1, t1 = correction(e, v, w, y, theta, 4, method_cheb(degree))
    assert np.isfinite(t1).all() and t1.any()

    def work(e, r):
        put(e)
        return correction(e, v, w, y, theta, 4, method_cheb(degree))

    for r3, t3 in three_ranks(n, 2 * m, work):
        assert np.array_equal(bits(r3), bits(r1)) and np.array_equal(bits(t3), bits(t1))


# ---- 6. solves ----------------------------------------------------------------------------------------------------------------------------------
def solve_inputs():
    t = I.table_inputs()
    return {"lap16": (t["lap16_l4"][0], 4, 4), "lap24": (t["lap24_l8"][0], 8, 4), "block240": (t["block240_b4"][0], 4, 4),
            "block256": (t["block256_b16"][0], 4, 16)}


def check_pairs(a, lam, vec, ref, tol=1e-8):
    assert np.linalg.norm(a @ vec - vec * lam[None, :], axis=0).max() < tol
    assert np.abs(lam - ref).max() < tol


def put_operator(eng, a, b, form):
    if form == "csr":
        eng.set_sparse(1, *I.csr_of(a))
    else:
        eng.set_block_sparse(1, *BI.bsr_of(a, b))


@pytest.mark.parametrize("form", ["csr", "bsr"])
@pytest.mark.parametrize("name", ["lap16", "lap24", "block240", "block256"])
def test_solves_converge_in_a_third_of_scalar_dprs_iterations(name, form):
    a, lowest, b = solve_inputs()[name]
    ref = np.linalg.eigvalsh(a)[:lowest]
    its = {}
    with fd.DavidsonEngine(a.shape[0], lowest) as eng:
        put_operator(eng, a, b, form)
        for method in ("CHEB", "DPR", "CHEB6", "CHEB16"):
            lam, vec, its[method] = eng.solve(method, I.MAX_ITERATIONS, 1e-8)
            assert its[method] <= I.MAX_ITERATIONS, (method, its)
            check_pairs(a, lam, vec, ref)
    print(f"{name} as {form}: iterations {its}")
    assert 3 * its["CHEB"] <= its["DPR"], its
    assert its["CHEB16"] <= its["CHEB6"], its


# ---- 7. policies, device-side Rayleigh-Ritz, warm start -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["csr", "bsr"])
@pytest.mark.parametrize("option", ["unconverged", "locking", "device_rr"])
def test_policies_and_device_rayleigh_ritz_reach_the_same_eigenvalues(option, form):
    a, lowest, b = solve_inputs()["lap16"]
    with fd.DavidsonEngine(a.shape[0], lowest) as eng:
        put_operator(eng, a, b, form)
        if option == "device_rr":
            eng.set_device_rr(True)
        else:
            eng.set_correction_policy(option)
        lam, vec, it = eng.solve("CHEB", I.MAX_ITERATIONS, 1e-8)
    assert it <= I.MAX_ITERATIONS, it
    check_pairs(a, lam, vec, np.linalg.eigvalsh(a)[:lowest])


def test_a_warm_started_second_solve():
    a, lowest, b = solve_inputs()["lap16"]
    ref = np.linalg.eigvalsh(a)[:lowest]
    with fd.DavidsonEngine(a.shape[0], lowest) as eng:
        eng.set_sparse(1, *I.csr_of(a))
        lam, vec, it = eng.solve("CHEB", I.MAX_ITERATIONS, 1e-8, reuse_vectors=True)
        check_pairs(a, lam, vec, ref)
        lam2, vec2, it2 = eng.solve("CHEB12", I.MAX_ITERATIONS, 1e-8)
    check_pairs(a, lam2, vec2, ref)
    assert it2 <= 2 < it, (it, it2)


# ---- 8. the one-call front ends and the Fortran program -----------------------------------------------------------------------------------------------
def test_the_one_call_front_ends_solve_with_cheb():
    a, lowest, b = solve_inputs()["block240"]
    ref = np.linalg.eigvalsh(a)[:lowest]
    lam, vec, it = fd.solver.generalized_eigensolver_sparse(*I.csr_of(a), lowest, "CHEB", 300, 1e-8)
    assert it <= 300
    check_pairs(a, lam, vec, ref)
    lam, vec, it16 = fd.solver.generalized_eigensolver_sparse(*I.csr_of(a, lower=True), lowest, "CHEB16", 300, 1e-8, lower=True)
    assert it16 <= it
    check_pairs(a, lam, vec, ref)
    lam, vec, it = fd.solver.generalized_eigensolver_bsr(*BI.bsr_of(a, b), lowest, "CHEB", 300, 1e-8)
    assert it <= 300
    check_pairs(a, lam, vec, ref)


def fortran_matrix(nx=16):
    """the matrix tests/fortran/prog_cheb.f90 builds, from the same integer formula"""
    a = I.laplacian2d(nx)
    n = nx * nx
    i = np.arange(1, n + 1)
    a[np.arange(n), np.arange(n)] = 4.0 + 0.05 * (((37 * i + 11) % 101) / 101.0 - 0.5)
    return a


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang not available")
def test_fortran_program_solves_with_cheb(tmp_path):
    from test_fortran_programs import SRC, _run, compile_link
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    exe = compile_link([os.path.join(SRC, "prog_cheb.f90")], os.path.join(bindir, "prog_cheb"), tmp_path)
    rc, out = _run(exe)
    assert rc == 0, out
    a = fortran_matrix()
    it_csr, it_bsr, it_16, it_dpr = [int(x) for x in re.search(r"ITERS\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", out).groups()]
    assert 3 * it_csr <= it_dpr <= 400 and 3 * it_bsr <= it_dpr and it_16 <= it_csr
    ref = np.linalg.eigvalsh(a)[:4]
    for label in ("EVALS_CSR", "EVALS_BSR", "EVALS_D16"):
        ev = np.array([float(x) for x in re.search(label + r"(.*)", out).group(1).split()])
        assert np.abs(ev - ref).max() < 1e-8, label
    checks = re.findall(r"CHECK (\S+) ([TF])", out)
    assert len(checks) == 12 and all(v == "T" for _, v in checks), out
