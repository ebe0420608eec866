"""The device Rayleigh-Ritz eigensolver (csrc/k_smalleig.hip: small_eig_kernel, rr_scatter_kernel, rr_pack_kernel) on the
hard and special spectra of tests/small_eig_inputs.py, at every class of order that has index arithmetic of its own
(powers of two and their neighbours, odd orders with a bye slot, 1-3, the LDS / global switch of the rotations between 97
and 98), against LAPACK in fp64 (and 50-digit arithmetic where LAPACK is no reference).

H and S reach the kernel EXACTLY: operator A = blockdiag(H, I), B = blockdiag(S, I), basis = unit columns.  A dense product
with unit columns and the Gram product of unit columns have one non-zero term per entry.  Every case asserts that.

Each case prints its figures (docs/small_eig_spectra.md is made from them)."""
import mpmath
import numpy as np
import pytest
import scipy.linalg

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import OP_A, OP_B, PANEL_V, PANEL_W, PANEL_BV
import small_eig_inputs as F

pytestmark = pytest.mark.gpu
METHOD_NONE = 2
N = 256
EPS = 2.0 ** -52
ALL = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 98, 127, 128]
SOME = [3, 8, 33, 64, 98, 128]
MAX_SWEEPS = 30
EV_TOL, ORTH_TOL, RES_TOL, GRADED_REL_TOL = 1e-12, 1e-12, 1e-13, 1e-11
EXACTLY_DIAGONAL = ("diagonal", "scaled_identity", "zero")
RANK_DEFICIENT = ("rank_one", "null_space")


def embed(X, n=N):
    A = np.eye(n)
    A[:X.shape[0], :X.shape[0]] = X
    return A


def unit_columns(m, first=0, n=N):
    V = np.zeros((n, m), order="F")
    V[first + np.arange(m), np.arange(m)] = 1.0
    return V


def load(e, H, S):
    """operators and basis such that the projected matrices are H and S themselves; returns what dav_project handed back"""
    m = H.shape[0]
    e.set_dense_host(OP_A, embed(H))
    if S is not None:
        e.set_dense_host(OP_B, embed(S))
    e.rr_enable(True)
    e.panel_put(PANEL_V, 0, unit_columns(m))
    e.apply(OP_A, PANEL_V, 0, m, PANEL_W, 0)
    if S is not None:
        e.apply(OP_B, PANEL_V, 0, m, PANEL_BV, 0)
    Ho, So = np.zeros((m, m), order="F"), np.zeros((m, m), order="F")
    e.project(0, m, Ho, So if S is not None else None)
    return Ho, So


def reload(e, H, S):
    """the same in an engine that already has its operators: the images W = A V and B V are put directly"""
    m = H.shape[0]
    e.panel_put(PANEL_V, 0, unit_columns(m))
    for panel, X in ((PANEL_W, H), (PANEL_BV, S)):
        if X is not None:
            W = np.zeros((N, m), order="F")
            W[:m, :] = X
            e.panel_put(panel, 0, W)
    Ho, So = np.zeros((m, m), order="F"), np.zeros((m, m), order="F")
    e.project(0, m, Ho, So if S is not None else None)
    return Ho, So


def decompose(H, S, repeat=True):
    """(theta, Y, sweeps, residual norms of the first L pairs); twice on the same input, which must agree bit for bit
    (the sweep flag is written by many threads: the number of sweeps must not depend on who wins)"""
    m = H.shape[0]
    L = min(3, m)
    with fd.CEngine(n=N, max_cols=128, gev=S is not None) as e:
        Ho, So = load(e, H, S)
        assert np.array_equal(Ho, H), "injection of H is no longer exact"
        assert S is None or np.array_equal(So, S), "injection of S is no longer exact"
        theta, res, sweeps = e.rr_ritz(m, m, L, METHOD_NONE)
        th2, Y = e.rr_get(m, m)
        assert np.array_equal(theta, th2)
        if repeat:
            theta_b, res_b, sweeps_b = e.rr_ritz(m, m, L, METHOD_NONE)
            th2_b, Y_b = e.rr_get(m, m)
            assert sweeps_b == sweeps and np.array_equal(theta_b, theta) and np.array_equal(Y_b, Y) and np.array_equal(res_b, res)
    return theta, Y, sweeps, res


def norm_inf(X):
    return np.abs(X).sum(axis=1).max()


def check_fused_residual_norms(H, S, theta, Y, res):
    """with unit basis columns the residual norms of the fused Ritz phase ARE ||H y - theta S y||_2 of the first L pairs: a
    second look at Y and theta through rr_pack_kernel and the panel product.  Two fp64 evaluations of a sum of m terms"""
    L = len(res)
    Sm = np.eye(len(H)) if S is None else S
    R = H @ Y[:, :L] - (Sm @ Y[:, :L]) * theta[None, :L]
    scale = (norm_inf(H) + np.abs(theta[:L]) * norm_inf(Sm)) * np.linalg.norm(Y[:, :L], axis=0)
    assert (np.abs(res - np.linalg.norm(R, axis=0)) <= 1e-12 * scale + 1e-300).all(), (res, np.linalg.norm(R, axis=0))


def report(name, m, gev, sweeps, everr, resid, orth, extra=""):
    print(f"\nSMALLEIG {name} {m} {'gev' if gev else 'std'} sweeps={sweeps} everr={everr:.1e} resid={resid:.1e} orth={orth:.1e} {extra}")


def check_case(name, H, S, label=None):
    m = H.shape[0]
    theta, Y, sweeps, res = decompose(H, S)
    ref = scipy.linalg.eigh(H, S, eigvals_only=True)
    scale = np.abs(ref).max()
    everr = np.abs(theta - ref).max() / scale if scale > 0 else np.abs(theta).max()
    resid, orth = F.scaled_residual(H, S, theta, Y), F.orthogonality(S, Y)
    report(label or name, m, S is not None, sweeps, everr, resid, orth)
    assert np.isfinite(theta).all() and np.isfinite(Y).all()
    assert (np.diff(theta) >= 0).all()
    assert np.abs(theta - ref).max() <= EV_TOL * scale
    assert orth <= ORTH_TOL
    assert resid <= RES_TOL
    check_fused_residual_norms(H, S, theta, Y, res)
    if m == 1 or (S is None and name in EXACTLY_DIAGONAL) or not H.any():
        assert sweeps == 0
    elif name in RANK_DEFICIENT:
        assert sweeps < MAX_SWEEPS
    else:
        assert 0 < sweeps < MAX_SWEEPS
    return theta, Y, sweeps


# ---- every order class: three kinds of H, standard and generalized ------------------------------------------------------
@pytest.mark.parametrize("gev", [False, True])
@pytest.mark.parametrize("m", ALL)
@pytest.mark.parametrize("name", ["indefinite", "diagonal", "two_values"])
def test_every_order_class(name, m, gev):
    H = F.FAMILIES[name](m, 0)[0]
    S = F.S_near_identity(m, 0)[1] if gev else None
    theta, Y, sweeps = check_case(name, H, S, label=name + ("+S_near_identity" if gev else ""))
    if name == "diagonal" and not gev:
        # the state after every restart: no rotation at all, the Ritz values are the diagonal entries themselves and Y the
        # permutation that sorts them
        d = np.diag(H)
        perm = np.argsort(d, kind="stable")
        assert np.array_equal(theta, d[perm])
        assert np.array_equal(Y, np.eye(m)[:, perm])


@pytest.mark.parametrize("m", SOME)
@pytest.mark.parametrize("name", ["scaled_identity", "zero"])
def test_equal_diagonal_entries_are_ordered_by_index(name, m):
    H = F.FAMILIES[name](m, 0)[0]
    theta, Y, sweeps = check_case(name, H, None)
    assert sweeps == 0 and np.array_equal(theta, np.diag(H)) and np.array_equal(Y, np.eye(m))


def test_repeated_diagonal_entries_are_ordered_by_index():
    """ties by index among DISTINCT groups: 2, 1, 2, 1, ... -> the ones in their order, then the twos in theirs"""
    for m in (3, 8, 33, 98):
        d = np.where(np.arange(m) % 2 == 0, 2.0, 1.0)
        theta, Y, sweeps, _ = decompose(np.diag(d), None)
        perm = np.argsort(d, kind="stable")
        assert sweeps == 0 and np.array_equal(theta, d[perm]) and np.array_equal(Y, np.eye(m)[:, perm])


@pytest.mark.parametrize("m", SOME)
@pytest.mark.parametrize("name", ["cluster", "graded_dense", "rank_one", "null_space", "scaled_down", "scaled_up", "wilkinson"])
def test_hard_spectra(name, m):
    H = F.FAMILIES[name](m, 0)[0]
    check_case(name, H, None)


@pytest.mark.parametrize("m", SOME)
def test_graded_scaled_keeps_the_relative_accuracy_of_every_eigenvalue(m):
    """D (I + 1e-2 E) D: Jacobi with the entrywise-relative criterion owes every eigenvalue 1e-11 of its OWN size.  The
    reference for that is 50-digit arithmetic (m <= 24; LAPACK is only norm-wise accurate here, the CPU test shows it);
    at every order the norm-wise checks against LAPACK hold as for any other family."""
    H = F.graded_scaled(m, 0)[0]
    theta, Y, sweeps = check_case("graded_scaled", H, None)
    if m <= 24:
        with mpmath.workdps(50):
            ev = mpmath.eigsy(mpmath.matrix(H.tolist()), eigvals_only=True)
            exact = np.array(sorted(float(ev[i]) for i in range(m)))
        rel = np.abs(theta - exact) / np.abs(exact)
        print(f"\nSMALLEIG graded_scaled {m} std relative-to-50-digits={rel.max():.1e}")
        assert (rel <= GRADED_REL_TOL).all()


@pytest.mark.parametrize("m", SOME)
def test_ill_conditioned_overlap_against_lapack_on_the_same_input(m):
    """S of condition 1e10: the Cholesky reduction loses digits, in LAPACK's DSYGV as here, so no bound is fixed in advance.
    LAPACK's scaled residual and orthogonality are measured on the same input and the device is allowed ten times each
    (floor 1e-13): both are backward-stable Cholesky reductions, and one decade covers the different summation order.

    Eigenvalues: 50-digit arithmetic shows (tests/test_small_eig_inputs_cpu.py) that LAPACK itself is off by 1e-7 of the
    largest eigenvalue here, so it is no reference at 1e-12.  The reduced matrix C = L^-1 H L^-T comes out of two triangular
    solves of condition cond(S), carries a forward error of eps cond(S) ||C||, and by Weyl every eigenvalue moves by at most
    that.  LAPACK sits ten times inside (CPU test); the difference of the two gets ten times the bound, and never less than
    the 1e-12 max|theta| of every other family."""
    H, S = F.S_cond1e10(m, 0)
    theta, Y, sweeps, res = decompose(H, S)
    ref, Yref = scipy.linalg.eigh(H, S)
    res_l, orth_l = F.scaled_residual(H, S, ref, Yref), F.orthogonality(S, Yref)
    res_d, orth_d = F.scaled_residual(H, S, theta, Y), F.orthogonality(S, Y)
    everr = np.abs(theta - ref).max() / np.abs(ref).max()
    report("S_cond1e10", m, True, sweeps, everr, res_d, orth_d, f"lapack_resid={res_l:.1e} lapack_orth={orth_l:.1e}")
    assert np.isfinite(theta).all() and np.isfinite(Y).all() and (np.diff(theta) >= 0).all()
    assert 0 < sweeps < MAX_SWEEPS
    assert res_d <= max(10.0 * res_l, 1e-13)
    assert orth_d <= max(10.0 * orth_l, 1e-13)
    assert np.abs(theta - ref).max() <= max(10.0 * EPS * np.linalg.cond(S), EV_TOL) * np.abs(ref).max()
    check_fused_residual_norms(H, S, theta, Y, res)


# ---- failures that must be reported -----------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 33, 98])
def test_late_and_zero_pivots_are_reported_and_the_engine_recovers(m):
    Hgood, Sgood = F.S_near_identity(m, 0)
    ref = scipy.linalg.eigh(Hgood, Sgood, eigvals_only=True)
    with fd.CEngine(n=N, max_cols=128, gev=True) as e:
        for bad, pivot in ((F.S_late_negative, m), (F.S_semidefinite, m // 2 + 1)):
            H, S = bad(m, 0)
            Ho, So = (load if bad is F.S_late_negative else reload)(e, H, S)
            assert np.array_equal(Ho, H) and np.array_equal(So, S)
            with pytest.raises(fd.DavidsonHipError, match=rf"positive definite \(pivot {pivot}\)"):
                e.rr_ritz(m, m, min(3, m), METHOD_NONE)
            # the same engine, a good overlap: a correct result
            Ho, So = reload(e, Hgood, Sgood)
            assert np.array_equal(Ho, Hgood) and np.array_equal(So, Sgood)
            theta, res, sweeps = e.rr_ritz(m, m, min(3, m), METHOD_NONE)
            th2, Y = e.rr_get(m, m)
            assert np.abs(theta - ref).max() <= EV_TOL * np.abs(ref).max()
            assert F.orthogonality(Sgood, Y) <= ORTH_TOL and F.scaled_residual(Hgood, Sgood, theta, Y) <= RES_TOL


@pytest.mark.parametrize("gev", [False, True])
@pytest.mark.parametrize("where,value", [("diagonal", np.nan), ("off_diagonal", np.nan), ("off_diagonal", np.inf), ("diagonal", -np.inf)])
def test_non_finite_projected_matrix_is_an_error_not_the_previous_result(where, value, gev):
    """a Davidson breakdown must not come back as the plausible Ritz values of the call before.  The non-finite number is
    put into the image panel W = A V, at the position of H's entry; through the Gram product it spreads over a column (and
    row) of H - the way a breakdown reaches the projected matrix in a solve."""
    m = 16
    H, S = F.S_near_identity(m, 0)
    if not gev:
        S = None
    i, j = (5, 5) if where == "diagonal" else (2, 9)
    with fd.CEngine(n=N, max_cols=128, gev=gev) as e:
        load(e, H, S)
        theta, res, sweeps = e.rr_ritz(m, m, 3, METHOD_NONE)              # a successful call: stale finite values exist
        assert np.isfinite(theta).all() and np.isfinite(e.rr_get(m, m)[0]).all()
        W = np.zeros((N, m), order="F")
        W[:m, :] = H
        W[i, j] = value
        e.panel_put(PANEL_W, 0, W)
        Ho, So = np.zeros((m, m), order="F"), np.zeros((m, m), order="F")
        e.project(0, m, Ho, So if gev else None)
        assert not np.isfinite(Ho[i, j])                                   # in the upper triangle, which the kernel reads
        with pytest.raises(fd.DavidsonHipError, match="projected matrix is not finite"):
            e.rr_ritz(m, m, 3, METHOD_NONE)
        assert not np.isfinite(e.rr_get(m, m)[0]).any()                    # no finite theta comes back
        # and the engine is usable afterwards
        reload(e, H, S)
        theta2, _, _ = e.rr_ritz(m, m, 3, METHOD_NONE)
        assert np.array_equal(theta2, theta)


# ---- rr_scatter_kernel: a projection cut into blocks is the projection in one block --------------------------------------
def _project_in_blocks(e, blocks):
    c0 = 0
    for k in blocks:
        e.project_dev(c0, k)
        c0 += k


@pytest.mark.parametrize("gev", [False, True])
def test_incremental_projection_is_bit_identical_to_one_block(gev):
    m = 40
    H, S = F.S_near_identity(m, 0)
    if not gev:
        S = None
    out = []
    for blocks in ((40,), (8, 8, 16, 8)):
        with fd.CEngine(n=N, max_cols=128, gev=gev) as e:
            e.set_dense_host(OP_A, embed(H))
            if gev:
                e.set_dense_host(OP_B, embed(S))
            e.rr_enable(True)
            e.panel_put(PANEL_V, 0, unit_columns(m))
            e.apply(OP_A, PANEL_V, 0, m, PANEL_W, 0)
            if gev:
                e.apply(OP_B, PANEL_V, 0, m, PANEL_BV, 0)
            _project_in_blocks(e, blocks)
            theta, res, sweeps = e.rr_ritz(m, m, 3, METHOD_NONE)
            out.append((theta, e.rr_get(m, m)[1], sweeps, res))
    (t1, Y1, s1, r1), (t2, Y2, s2, r2) = out
    assert s1 == s2 and np.array_equal(t1, t2) and np.array_equal(Y1, Y2) and np.array_equal(r1, r2)
    ref = scipy.linalg.eigh(H, S, eigvals_only=True)
    assert np.abs(t1 - ref).max() <= EV_TOL * np.abs(ref).max()


@pytest.mark.parametrize("gev", [False, True])
def test_projection_after_a_shrink_is_bit_identical_to_a_fresh_engine(gev):
    """order 40, collapse to the 8 lowest Ritz vectors (now DENSE columns: the Gram sums round), grow again to 24 in blocks of
    8 and 16 over what the resident matrices still hold of order 40 - against a fresh engine, whose resident matrices hold
    nothing, given the same 24 columns"""
    m, keep, grow = 40, 8, 16
    H, S = F.S_near_identity(m + grow, 0)
    if not gev:
        S = None
    panels = [PANEL_V, PANEL_W] + ([PANEL_BV] if gev else [])
    with fd.CEngine(n=N, max_cols=128, gev=gev) as e:
        e.set_dense_host(OP_A, embed(H))
        if gev:
            e.set_dense_host(OP_B, embed(S))
        e.rr_enable(True)
        e.panel_put(PANEL_V, 0, unit_columns(m))
        e.apply(OP_A, PANEL_V, 0, m, PANEL_W, 0)
        if gev:
            e.apply(OP_B, PANEL_V, 0, m, PANEL_BV, 0)
        e.project_dev(0, m)
        e.rr_ritz(m, m, 3, METHOD_NONE)
        e.rr_restart(m, keep)
        e.panel_put(PANEL_V, keep, unit_columns(grow, first=m))           # orthogonal to everything kept
        e.apply(OP_A, PANEL_V, keep, grow, PANEL_W, keep)
        if gev:
            e.apply(OP_B, PANEL_V, keep, grow, PANEL_BV, keep)
        _project_in_blocks(e, (keep, grow))
        theta, res, sweeps = e.rr_ritz(keep + grow, keep + grow, 3, METHOD_NONE)
        Y = e.rr_get(keep + grow, keep + grow)[1]
        cols = [e.panel_get(p, 0, keep + grow) for p in panels]
    with fd.CEngine(n=N, max_cols=128, gev=gev) as e:
        e.set_dense_host(OP_A, embed(H))
        if gev:
            e.set_dense_host(OP_B, embed(S))
        e.rr_enable(True)
        for p, c in zip(panels, cols):
            e.panel_put(p, 0, c)
        _project_in_blocks(e, (keep, grow))     # the same Gram launches: dense columns, whose sums depend on the tile shape
        theta_f, res_f, sweeps_f = e.rr_ritz(keep + grow, keep + grow, 3, METHOD_NONE)
        Y_f = e.rr_get(keep + grow, keep + grow)[1]
    assert sweeps == sweeps_f and np.array_equal(theta, theta_f) and np.array_equal(Y, Y_f) and np.array_equal(res, res_f)
    # and it is the Rayleigh-Ritz of those 24 columns
    V = cols[0]
    Hp = V.T @ embed(H) @ V
    Sp = V.T @ embed(S) @ V if gev else None
    ref = scipy.linalg.eigh(0.5 * (Hp + Hp.T), None if Sp is None else 0.5 * (Sp + Sp.T), eigvals_only=True)
    assert np.abs(theta - ref).max() <= EV_TOL * np.abs(ref).max()
