"""GPU: the Chebyshev-filtered correction with a Lanczos bound (method "LCHEB", DAV_METHOD_LCHEB; the Lanczos kernels in
fortran_davidson_amd/csrc/k_lanczos.hip, the run in engine_cheb.hip).  The engine's bound, read out of a degree-1 block, against the numpy
restatement for every kind of operator; when it is built and built again; the correction block against the restatement in long double
with the engine's own bound; the refusals and the degenerate interval; solves against eigvalsh, scalar DPR's iteration counts and the
restated counts; three ranks against one; policies and the device-side Rayleigh-Ritz."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import (METHOD_DPR, METHOD_LCHEB, OP_A, OP_B, PANEL_BV, PANEL_R, PANEL_V, PANEL_W, DavidsonHipError, method_lcheb)
import bdpr_inputs as BI
import cheb_inputs as CI
import lcheb_inputs as I
from test_bdpr_gpu import PadRows, bits, set_bsr, three_ranks
from test_cheb_gpu import check_block, check_pairs, correction, ritz_pairs

pytestmark = pytest.mark.gpu
U = I.U
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHOD_NONE = 2


@pytest.fixture(scope="module")
def user():
    fd.hip_lib()            # first: one HIP runtime per process (the helper follows the engine's)
    lib = C.CDLL(os.path.join(ROOT, "fortran_davidson_amd", "lib", "test", "libuser_operator.so"))
    lib.user_op_create.restype = C.c_void_p
    lib.user_op_create.argtypes = [C.c_double, C.c_double, C.c_double]
    lib.user_op_destroy.argtypes = [C.c_void_p]
    return lib


def set_stencil(e, user, n, d0, dstep, eps, which=OP_A):
    """the stencil of tests/helpers/user_operator.hip as the device callback of a CEngine (the context lives as long as the process)"""
    ctx = user.user_op_create(d0, dstep, eps)
    e.set_operator_device(which, user.user_op_apply, ctx, d0 + dstep * np.arange(n, dtype=np.float64))


# ---- inputs, computed once ------------------------------------------------------------------------------------------------------------
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def sparse_matrix(n, seed):
    """about seven entries per row, a nearly flat diagonal, both signs (test_cheb_gpu's)"""
    return cached(("sparse", n, seed), lambda: CI.random_sparse(n, 6.0 / n, seed, grade=0.5 / n))


def restated_bound(key, a):
    return cached(("bound", key), lambda: I.lanczos_bound(a))


# name -> (matrix, how a CEngine takes it)
def operator_kinds(user):
    stencil = I.stencil_matrix(500, 3.0, 0.0, -1.0)
    band = I.stencil_matrix(777, 3.0, 1e-3, -1.0)
    blocks = BI.block_matrix(300, 3, 23)[0]

    def dense(a, storage):
        def put(e):
            e.set_storage(storage)
            e.set_dense_host(OP_A, np.asfortranarray(a))
        return put
    return {
        "dense_full": (sparse_matrix(301, 5), dense(sparse_matrix(301, 5), 0)),
        "dense_symmetric": (sparse_matrix(301, 5), dense(sparse_matrix(301, 5), 1)),
        "csr": (sparse_matrix(777, 777), lambda e: e.set_operator_csr(OP_A, *CI.csr_of(sparse_matrix(777, 777)))),
        "bsr3": (blocks, lambda e: set_bsr(e, OP_A, BI.bsr_of(blocks, 3))),
        "dia": (band, lambda e: e.set_operator_csr(OP_A, *CI.csr_of(band), diagonals=True)),
        "stencil": (stencil, lambda e: set_stencil(e, user, 500, 3.0, 0.0, -1.0)),
    }


def bound_panels(n, near):
    """two columns and two Ritz values that make the first coefficient of a degree-1 block a sensitive function of the bound: a0 = 0.5,
    a = 0.6 of about the bound, so that alpha_0 = -2 / (a + b - 2 a0) moves 1.7 units in the last place per unit of b"""
    rng = np.random.default_rng(n)
    v = np.asfortranarray(rng.standard_normal((n, 2)))
    w = np.asfortranarray(rng.standard_normal((n, 2)))
    return v, w, np.array([0.5 * near, 0.6 * near])


def engine_bounds(e, n, near):
    """every double the engine's bound can be, from a degree-1 correction: t = alpha_0 r, alpha_0 a function of b and theta
    (lcheb_inputs.first_coefficient).  near: about the bound.  Returns (the ascending array of doubles, the block)."""
    v, w, theta = bound_panels(n, near)
    r, t = correction(e, v, w, np.eye(2, order="F"), theta, 1, method_lcheb(1))
    assert np.isfinite(t).all() and t.any()
    c = I.coefficient_of_block(r, t)
    assert isinstance(c, float), ("the block is not one coefficient times R", c)
    found = I.bounds_giving(c, theta, 2, 1, near)
    assert found.size, "no bound near the restatement gives the engine's coefficient"
    return found, t


def ulps_off(found, want):
    """the largest |b - want| / (u want) over the doubles b the engine's bound can be"""
    return float(np.abs(found - want).max() / (U * abs(want)))


# ---- 1. the bound -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense_full", "dense_symmetric", "csr", "bsr3", "dia", "stencil"])
def test_the_bound_equals_the_restatement(user, kind):
    """... to 64 u relative, the allowance for the order of the dot products; a second correction adds d - 1 applies only"""
    a, put = operator_kinds(user)[kind]
    n = a.shape[0]
    want = restated_bound(kind, a)
    assert want >= np.linalg.eigvalsh(a).max()
    with fd.CEngine(n=n, max_cols=32) as e:
        put(e)
        e.reset_stats()
        found, _ = engine_bounds(e, n, want)
        off = ulps_off(found, want)
        print(f"{kind} n={n}: the engine's bound is within {off:.1f} u of the restatement {want!r} ({found.size} candidate doubles)")
        assert e.stats().applies == I.STEPS and e.stats().apply_cols == I.STEPS          # degree 1: the Lanczos run alone
        assert off <= 64.0, (kind, off)
        # the bound is kept: degree 5 costs four block products, twice
        m, degree = 8, 5
        v, w, y, theta = ritz_pairs(("lcheb", kind), a, m, 11)
        for _ in range(2):
            before = e.stats().applies
            correction(e, v, w, y, theta, 4, method_lcheb(degree))
            assert e.stats().applies - before == degree - 1


def test_new_values_and_a_new_set_call_rebuild_the_bound(user):
    n = 300
    a1 = sparse_matrix(n, 1)
    a2 = np.where(a1 != 0.0, 1.75 * a1, 0.0) + np.diag(0.3 * np.cos(np.arange(n)))          # same pattern, another spectrum
    a3 = I.stencil_matrix(n, 3.0, 0.0, -1.0)
    arr1, arr2 = CI.csr_of(a1), CI.csr_of(a2)
    assert np.array_equal(arr1[0], arr2[0]) and np.array_equal(arr1[1], arr2[1])
    b1, b2, b3 = (I.lanczos_bound(a) for a in (a1, a2, a3))
    assert abs(b2 - b1) > 1e-3 * b1 and abs(b3 - b2) > 1e-3 * b2
    with fd.CEngine(n=n, max_cols=32) as e:
        e.keep_value_map(OP_A)
        e.set_operator_csr(OP_A, *arr1)
        e.reset_stats()
        assert ulps_off(engine_bounds(e, n, b1)[0], b1) <= 64.0 and e.stats().applies == I.STEPS
        e.update_operator_values(OP_A, arr2[2])
        assert ulps_off(engine_bounds(e, n, b2)[0], b2) <= 64.0 and e.stats().applies == 2 * I.STEPS
        assert ulps_off(engine_bounds(e, n, b2)[0], b2) <= 64.0 and e.stats().applies == 2 * I.STEPS      # kept
        set_stencil(e, user, n, 3.0, 0.0, -1.0)                                                            # a set call on slot A
        assert ulps_off(engine_bounds(e, n, b3)[0], b3) <= 64.0 and e.stats().applies == 3 * I.STEPS
        e.set_dense_host(OP_A, np.asfortranarray(a1))
        assert ulps_off(engine_bounds(e, n, b1)[0], b1) <= 64.0 and e.stats().applies == 4 * I.STEPS
        # streamed rows of a dense operator
        e.dense_begin(OP_A)
        e.dense_put_rows(OP_A, 0, a2)
        e.dense_end(OP_A)
        assert ulps_off(engine_bounds(e, n, b2)[0], b2) <= 64.0 and e.stats().applies == 5 * I.STEPS


# ---- 2. the correction block against the restatement in long double ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [50, 301, 777])
def test_the_block_matches_the_restatement_with_the_engines_bound(user, n):
    """test 1 of test_cheb_gpu.py - the same error figure and cap (check_block) - with the bound the engine itself holds"""
    a_dense = sparse_matrix(n, n)
    a_stencil = I.stencil_matrix(n, 3.0, 1e-3, -1.0)
    with fd.CEngine(n=n, max_cols=32) as e:
        pads = PadRows(e, n)
        for kind, a in (("dense_full", a_dense), ("dense_symmetric", a_dense), ("stencil", a_stencil)):
            if kind == "stencil":
                set_stencil(e, user, n, 3.0, 1e-3, -1.0)
            else:
                e.set_storage(1 if kind == "dense_symmetric" else 0)
                e.set_dense_host(OP_A, np.asfortranarray(a))
            found, _ = engine_bounds(e, n, restated_bound((kind, n), a))
            bound = float(found[found.size // 2])
            prod, worst = CI.Product(a), 0.0
            for m in (1, 5, 16):
                v, w, y, theta = ritz_pairs(("lcheb", kind, n), a, m, 1000 + m)
                lowest = min(4, m)
                r0, _ = correction(e, v, w, y, theta, lowest, METHOD_NONE)
                for degree in (1, 2, 3, 12):
                    pads.dirty(m, m)
                    r, t = correction(e, v, w, y, theta, lowest, method_lcheb(degree))
                    where = (kind, n, m, degree)
                    assert np.array_equal(bits(r), bits(r0)), where                      # R as the residual product wrote it
                    assert np.array_equal(bits(e.panel_get(PANEL_V, 0, m)), bits(v)), where
                    worst = max(worst, check_block(a, prod, bound, r, t, theta, m, lowest, degree, where))
                    assert not bits(pads.read(m, m)).any(), (where, "pad rows of the written columns are not +0.0")
            print(f"{kind} n={n}: largest error / bar = {worst:.3f}")


# ---- 3. refusals and the degenerate interval --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["generalized", "a_host", "a_unset", "degree_65"])
def test_what_the_method_does_not_serve_is_refused(case):
    n, m = 240, 5
    a = sparse_matrix(n, 3)
    v, w, y, theta = ritz_pairs("lcheb_refuse", a, m, 4)
    method = METHOD_LCHEB
    with fd.CEngine(n=n, max_cols=16, gev=case == "generalized") as e:
        if case == "generalized":
            e.set_dense_host(OP_A, np.asfortranarray(a))
            e.set_dense_host(OP_B, np.asfortranarray(np.eye(n)))
            want = "generalized problem"
        elif case == "a_host":
            e.set_operator_host(OP_A, np.diag(a).copy())
            want = "operator A is a host callback"
        elif case == "a_unset":
            want = "operator A is not set"
        else:
            e.set_dense_host(OP_A, np.asfortranarray(a))
            method, want = method_lcheb(65), "degree 65 is outside 1..64"
        mark = np.full((n, m), 3.25)
        e.panel_put(PANEL_V, m, mark)
        e.panel_put(PANEL_R, 0, mark)
        e.panel_put(PANEL_V, 0, v)
        e.panel_put(PANEL_W, 0, w)
        e.reset_stats()
        with pytest.raises(DavidsonHipError, match=re.escape(want)) as exc:
            e.ritz_residual_correction(m, 4, y, theta, method)
        assert str(exc.value).startswith("LCHEB correction: ")
        assert e.stats().applies == 0
        assert np.array_equal(bits(e.panel_get(PANEL_V, 0, m)), bits(v)) and np.array_equal(bits(e.panel_get(PANEL_W, 0, m)), bits(w))
        assert np.array_equal(e.panel_get(PANEL_V, m, m), mark) and np.array_equal(e.panel_get(PANEL_R, 0, m), mark)
        if case != "a_unset":
            # the engine stays usable: scalar DPR on the same panels
            if case == "generalized":
                e.panel_put(PANEL_BV, 0, v)            # BV = I V
            _, t = correction(e, v, w, y, theta, 4, METHOD_DPR)
            assert np.isfinite(t).all()


@pytest.mark.parametrize("storage", [0, 1])
def test_a_zero_matrix_gives_a_zero_block(storage):
    n, m = 300, 5
    v = np.asfortranarray(np.linalg.qr(np.random.default_rng(0).standard_normal((n, m)))[0])
    w = np.zeros((n, m), order="F")
    with fd.CEngine(n=n, max_cols=16) as e:
        pads = PadRows(e, n)
        e.set_storage(storage)
        e.set_dense_host(OP_A, np.zeros((n, n), order="F"))                          # b = 0 = a0
        e.panel_put(PANEL_V, m, np.full((n, m), 3.25))
        pads.dirty(m, m)
        e.reset_stats()
        r, t = correction(e, v, w, np.eye(m), np.zeros(m), 4, METHOD_LCHEB)
        assert not bits(t).any() and not bits(pads.read(m, m)).any()                 # +0.0, not -0.0
        assert not r.any()
        assert e.stats().applies == 1 + CI.DEFAULT_DEGREE - 1                        # the run stops at its first step: beta = 0


# ---- 4. solves --------------------------------------------------------------------------------------------------------------------------
def put_solve_operator(eng, user, name, form, a, keep):
    if form == "stencil":
        ctx = user.user_op_create(3.0, 1e-3, -1.0)
        keep.append(ctx)
        eng.set_device_operator(1, user.user_op_apply, ctx, 3.0 + 1e-3 * np.arange(eng.n, dtype=np.float64))
    elif form in ("dense_full", "dense_symmetric"):
        eng.set_dense(1, a)
    elif form == "csr":
        eng.set_sparse(1, *CI.csr_of(a))
    else:
        eng.set_block_sparse(1, *BI.bsr_of(a, 4))


SOLVES = [("stencil300_l4", "stencil"), ("stencil300_l8", "stencil"), ("noisy_lap16_l4", "dense_full"), ("noisy_lap16_l4", "dense_symmetric"),
          ("lap24_l8", "csr"), ("block240_b4", "bsr")]


@pytest.mark.parametrize("name,form", SOLVES)
def test_solves_converge_in_a_third_of_scalar_dprs_iterations(user, name, form):
    """... and, where the restatement models the engine, in its iterations (lcheb_inputs.TABLE) to one iteration.  Measured, engine
    against restatement, as LCHEB6 / LCHEB / LCHEB16 / DPR:
      stencil, lowest 4      28 / 18 / 14 / 207   against  30 / 20 / 14 / 203
      stencil, lowest 8      18 / 15 / 11 / 130   against  28 / 19 / 14 / 134
      dense full             18 / 11 /  7 / 123   against  18 / 11 /  7 / 123
      dense symmetric        18 / 11 /  7 / 126   against  18 / 11 /  7 / 123
      CSR 24 x 24            18 / 11 /  7 / 166   against  18 / 11 /  7 / 166
      BSR block240           16 / 10 /  7 /  56   against  16 / 10 /  7 /  56
    The stencil rows differ by more than one iteration, and the engine is the faster one.  The cause is not the correction: the
    blocks [V T] of the stencil are rank deficient from the second iteration on (unit start vectors at one end of a band; shown without
    a GPU by test_lcheb_cpu.py: test_the_stencils_blocks_are_rank_deficient_and_the_others_are_not), and the engine fills dependent
    columns with unit vectors at the next entries of the start order (davidson_ortho), which reach further along the band than the
    completion of the oracle's Householder QR.  The restatement is no model of the engine there, so those rows are held to what does
    not depend on the completion - convergence, the eigenvalues, a third of DPR's iterations - and their counts are printed.  Scalar
    DPR's hundreds of iterations are printed for every row: the engine's own two dense storages differ by three on one matrix."""
    a, lowest = cached(("table", name), lambda: I.table_inputs()[name])
    ref = np.linalg.eigvalsh(a)[:lowest]
    its, keep = {}, []
    with fd.DavidsonEngine(a.shape[0], lowest, storage="symmetric" if form == "dense_symmetric" else "full") as eng:
        put_solve_operator(eng, user, name, form, a, keep)
        for method in ("LCHEB", "DPR", "LCHEB6", "LCHEB16"):
            lam, vec, its[method] = eng.solve(method, I.MAX_ITERATIONS, 1e-8)
            assert its[method] <= I.MAX_ITERATIONS, (method, its)
            check_pairs(a, lam, vec, ref)
            assert np.abs(lam - ref).max() < 1e-9
    for ctx in keep:
        user.user_op_destroy(ctx)
    dpr, d6, d10, d16 = I.TABLE[name]
    print(f"{name} as {form}: iterations {its}, restated DPR / 6 / 10 / 16 = {I.TABLE[name]}")
    assert 3 * its["LCHEB"] <= its["DPR"] and 3 * its["LCHEB16"] <= its["DPR"], its
    assert its["LCHEB16"] <= its["LCHEB6"], its
    if form != "stencil":
        for method, want in (("LCHEB6", d6), ("LCHEB", d10), ("LCHEB16", d16)):
            assert abs(its[method] - want) <= 1, (name, form, method, its, I.TABLE[name])


def test_the_one_call_front_end_and_the_generated_operators_solve_with_lcheb():
    a, lowest = cached(("table", "noisy_lap16_l4"), lambda: I.table_inputs()["noisy_lap16_l4"])
    ref = np.linalg.eigvalsh(a)[:lowest]
    lam, vec, it = fd.solver.generalized_eigensolver(a, lowest, "LCHEB", 300, 1e-8)
    assert it <= 300
    check_pairs(a, lam, vec, ref)
    n = 400
    h = fd.solver.generate_diagonal_dominant(n, 1e-3)
    with fd.DavidsonEngine(n, 3) as eng:
        eng.set_hashed_operator(1, 1e-3)
        lam, vec, it = eng.solve("LCHEB16", 300, 1e-8)
    assert it <= 300
    check_pairs(h, lam, vec, np.linalg.eigvalsh(h)[:3])


# ---- 5. three ranks against one ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["stencil", "csr"])
def test_three_ranks_hold_one_bound_and_match_one_rank(user, kind):
    n = 301                                               # 112 rows on ranks 0 and 1, 77 on rank 2
    a = I.stencil_matrix(n, 3.0, 1e-3, -1.0) if kind == "stencil" else sparse_matrix(n, 2)
    want = restated_bound(("ranks", kind), a)

    def put(e):
        if kind == "stencil":
            set_stencil(e, user, n, 3.0, 1e-3, -1.0)
        else:
            e.set_operator_csr(OP_A, *CI.csr_of(a))

    with fd.CEngine(n=n, max_cols=32) as e:
        put(e)
        one, _ = engine_bounds(e, n, want)

    def work(e, r):
        put(e)
        return engine_bounds(e, n, want)

    out = three_ranks(n, 32, work)
    # Every rank computes the rows of its own slab with its own copy of the bound, and a panel comes back gathered: one coefficient
    # reproduces all n rows bit for bit (engine_bounds) only if the three ranks hold the same coefficient; the coefficient moves 1.7
    # units in the last place per unit of the bound
    for found, t in out:
        assert np.array_equal(found, out[0][0]) and np.array_equal(bits(t), bits(out[0][1]))
    three = out[0][0]
    gap = float(max(abs(three.max() - one.min()), abs(one.max() - three.min())) / (U * want))
    print(f"{kind}: three ranks against one: {gap:.1f} u; against the restatement: {ulps_off(three, want):.1f} u")
    assert gap <= 64.0 and ulps_off(three, want) <= 64.0


@pytest.mark.parametrize("kind", ["stencil", "csr"])
def test_three_ranks_solve_to_the_same_eigenvalues(user, kind):
    n, lowest, nranks = 301, 4, 3
    a = I.stencil_matrix(n, 3.0, 1e-3, -1.0) if kind == "stencil" else sparse_matrix(n, 2)
    keep = []

    def put(eng):
        if kind == "stencil":
            put_solve_operator(eng, user, None, "stencil", a, keep)
        else:
            eng.set_sparse(1, *CI.csr_of(a))

    with fd.DavidsonEngine(n, lowest) as eng:
        put(eng)
        lam1, vec1, it1 = eng.solve("LCHEB", I.MAX_ITERATIONS, 1e-8)
    check_pairs(a, lam1, vec1, np.linalg.eigvalsh(a)[:lowest])
    engs = [fd.DavidsonEngine(n, lowest, rank=r, nranks=nranks) for r in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.c.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def work(r):
        try:
            put(engs[r])
            out[r] = engs[r].solve("LCHEB", I.MAX_ITERATIONS, 1e-8, want_vectors=False)
        except Exception as exc:      # noqa: BLE001
            err[r] = exc
        finally:
            fd.hip_lib().dav_local_group_yield(engs[r].c.h)

    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join() for t in th]
    for e in engs:
        e.close()
    for ctx in keep:
        user.user_op_destroy(ctx)
    assert all(x is None for x in err), err
    for lam, _, it in out:
        assert it <= I.MAX_ITERATIONS and np.abs(lam - lam1).max() < 1e-9, (it, it1)


# ---- 6. policies and the device-side Rayleigh-Ritz --------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", ["unconverged", "locking", "device_rr"])
def test_policies_and_device_rayleigh_ritz_reach_the_same_eigenvalues(user, option):
    a, lowest = cached(("table", "stencil300_l4"), lambda: I.table_inputs()["stencil300_l4"])
    keep = []
    with fd.DavidsonEngine(a.shape[0], lowest) as eng:
        put_solve_operator(eng, user, None, "stencil", a, keep)
        if option == "device_rr":
            eng.set_device_rr(True)
        else:
            eng.set_correction_policy(option)
        lam, vec, it = eng.solve("LCHEB", I.MAX_ITERATIONS, 1e-8)
    for ctx in keep:
        user.user_op_destroy(ctx)
    assert it <= I.MAX_ITERATIONS, it
    check_pairs(a, lam, vec, np.linalg.eigvalsh(a)[:lowest])
