"""GPU: the block-diagonal preconditioned correction (method "BDPR", DAV_METHOD_BDPR; kernels in fortran_davidson_amd/csrc/k_bdpr.hip).
The kernel against the residues it read, by the backward error of Gaussian elimination with partial pivoting; exactly zero pivots;
b = 1 against scalar DPR bit for bit; new values on a kept pattern; the refusals; three ranks against one; solves against eigh and
against scalar DPR's iteration counts; the Fortran program."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import (BSR_COL_MAJOR, BSR_ROW_MAJOR, DEVICE_APPLY_FN, METHOD_BDPR, METHOD_DPR, OP_A, OP_B, PANEL_BV,
                                           PANEL_R, PANEL_V, PANEL_W, PANEL_X, DavidsonHipError)
import bdpr_inputs as I

pytestmark = pytest.mark.gpu
U = I.U


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def eigh_lowest(a, b, k):
    if b is None:
        return np.linalg.eigvalsh(a)[:k]
    l = np.linalg.cholesky(b)                      # B = L L^T: the eigenvalues of L^-1 A L^-T
    return np.linalg.eigvalsh(np.linalg.solve(l, np.linalg.solve(l, a).T))[:k]


def set_bsr(e, which, arrays, lower=False, colmajor=False):
    rp, ci, vv = arrays
    if colmajor:
        e.set_operator_bsr(which, rp, ci, np.ascontiguousarray(vv.transpose(0, 2, 1)), lower=lower, layout=BSR_COL_MAJOR)
    else:
        e.set_operator_bsr(which, rp, ci, vv, lower=lower, layout=BSR_ROW_MAJOR)


def correction(e, m, v, w, bv, theta, method):
    """the Ritz phase with Y = I on the panels V, W (and BV): returns (R, T) - for DPR, which writes no R, (None, T)"""
    e.panel_put(PANEL_V, 0, v[:, :m])
    e.panel_put(PANEL_W, 0, w[:, :m])
    if bv is not None:
        e.panel_put(PANEL_BV, 0, bv[:, :m])
    e.ritz_residual_correction(m, 1, np.eye(m), theta[:m], method)
    r = e.panel_get(PANEL_R, 0, m) if method == METHOD_BDPR else None
    return r, e.panel_get(PANEL_V, m, m)


def panels(n, m, seed, gev):
    rng = np.random.default_rng(seed)
    v, w = rng.standard_normal((n, m)), rng.standard_normal((n, m))
    bv = rng.standard_normal((n, m)) if gev else None
    theta = np.sort(rng.uniform(-3.0, 3.0, m))
    return v, w, bv, theta


class PadRows:
    """The pad rows [n, ld) of the engine's basis panel, which no panel door moves.  The engine hands a caller's device operator the
    address and the leading dimension of the panel it is to fill: an operator that only notes them down gives the test the panel, and
    the HIP runtime reads and writes the rows behind row n there.  (Made before the BSR operators are set.)"""

    def __init__(self, e, n):
        self.e, self.n, seen = e, n, []
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
        self.fn = DEVICE_APPLY_FN(lambda ctx, stream, nn, row0, nloc, k, x_dev, ldx, y_dev, ldy: seen.append((y_dev, ldy)) or 0)
        e.set_operator_device(OP_A, self.fn, 0, np.ones(n))
        e.apply(OP_A, PANEL_X, 0, 1, PANEL_V, 0)
        self.addr, self.ld = seen[-1]
        self.npad = self.ld - n
        assert self.npad > 0

    def _at(self, c0):
        return self.addr + 8 * (c0 * self.ld + self.n)

    def dirty(self, c0, ncols):
        self.e.synchronize()
        junk = np.full((ncols, self.npad), 7.0)
        assert self.hip.hipMemcpy2D(self._at(c0), 8 * self.ld, junk.ctypes.data, 8 * self.npad, 8 * self.npad, ncols, 1) == 0

    def read(self, c0, ncols):
        self.e.synchronize()
        out = np.full((ncols, self.npad), np.nan)
        assert self.hip.hipMemcpy2D(out.ctypes.data, 8 * self.npad, self._at(c0), 8 * self.ld, 8 * self.npad, ncols, 2) == 0
        return out


# ---- 1. the kernel against its own R, by backward error --------------------------------------------------------------------------------
def gamma(k):
    return k * U / (1.0 - k * U)


def backward_error_ratio(da, db, theta, r, t):
    """max over blocks and columns of ||r - M t||_inf / ((b^2 gamma_3b rho + 2u) ||M||_inf ||t||_inf), M = theta_j B_II - A_II formed
    exactly (extended precision) from the diagonal blocks the test summed; rho: the growth factor of the test's own elimination of M
    (Higham, Accuracy and Stability of Numerical Algorithms, theorem 9.5); 2u: the rounding of M's entries in the kernel"""
    nb, b, _ = da.shape
    m = r.shape[1]
    bI = np.broadcast_to(np.eye(b), da.shape) if db is None else db
    ml = theta[:m, None, None, None].astype(np.longdouble) * bI[None].astype(np.longdouble) - da[None].astype(np.longdouble)
    rl = r.T.reshape(m, nb, b).astype(np.longdouble)
    tl = t.T.reshape(m, nb, b).astype(np.longdouble)
    resid = np.abs(rl - np.einsum("jiab,jib->jia", ml, tl)).max(axis=2)
    mnorm = np.abs(ml).sum(axis=3).max(axis=2)
    tnorm = np.abs(tl).max(axis=2)
    m64 = ml.astype(np.float64).reshape(m * nb, b, b)
    _, rho, singular = I.eliminate_batch(m64, r.T.reshape(m * nb, b))
    assert not singular.any()
    bound = (b * b * gamma(3 * b) * rho.reshape(m, nb) + 2 * U) * mnorm * tnorm
    assert (tnorm > 0).all()
    return float((resid / bound).max())


@pytest.mark.parametrize("gev", [False, True], ids=["standard", "generalized"])
@pytest.mark.parametrize("b", [1, 2, 3, 4, 5, 7, 8, 12, 16])
def test_block_solves_are_backward_stable(b, gev):
    n = b * -(-300 // b)                     # the local rows cross one 256-row pad boundary
    a, bm = I.block_matrix(n, b, 10 + b, gev)
    worst = 0.0
    with fd.CEngine(n=n, max_cols=66, gev=gev) as e:
        pads = PadRows(e, n)
        for lower in (False, True):
            for colmajor in (False, True):
                for split in (None, 5):
                    arr_a = I.bsr_of(a, b, lower=lower, split=split)
                    arr_b = I.bsr_of(bm, b, lower=lower, split=split) if gev else None
                    set_bsr(e, OP_A, arr_a, lower, colmajor)
                    if gev:
                        set_bsr(e, OP_B, arr_b, lower, colmajor)
                    da = I.diagonal_blocks(*arr_a)
                    db = I.diagonal_blocks(*arr_b) if gev else None
                    assert np.array_equal(bits(e.get_diagonal(OP_A)), bits(np.einsum("iaa->ia", da).reshape(-1)))
                    for m in (1, 5, 16, 33):
                        v, w, bv, theta = panels(n, m, 100 * b + m, gev)
                        pads.dirty(m, m)
                        r, t = correction(e, m, v, w, bv, theta, METHOD_BDPR)
                        assert np.allclose(r, w - (bv if gev else v) * theta[None, :], rtol=0, atol=1e-13)
                        assert np.array_equal(bits(e.panel_get(PANEL_V, 0, m)), bits(v))
                        ratio = backward_error_ratio(da, db, theta, r, t)
                        worst = max(worst, ratio)
                        assert ratio <= 1.0, (b, gev, lower, colmajor, split, m, ratio)
                        assert not bits(pads.read(m, m)).any(), (b, gev, m, "pad rows of the written columns are not +0.0")
    print(f"b={b} gev={gev}: largest backward error / bound = {worst:.3e}")


# ---- 2. zero pivots, exactly ------------------------------------------------------------------------------------------------------------
def test_zero_pivots_give_zero_blocks():
    b, n, m = 2, 300, 2
    a, _ = I.block_matrix(n, b, 3)
    a0 = a.copy()
    a0[10:12, 10:12] = 0.0                           # an explicitly stored all-zero diagonal block
    a0[18:20, 18:20] = 1.0                           # [[1, 1], [1, 1]]: with theta = 0 the second pivot is exactly zero
    v, w, _, _ = panels(n, m, 1, False)
    theta = np.array([0.0, 0.7])
    out = []
    with fd.CEngine(n=n, max_cols=8) as e:
        for mat in (a, a0):
            set_bsr(e, OP_A, I.bsr_of(mat, b))
            out.append(correction(e, m, v, w, None, theta, METHOD_BDPR))
    (r1, t1), (r0, t0) = out
    assert np.array_equal(bits(r1), bits(r0))        # the residues do not depend on the operator
    for rows in (slice(10, 12), slice(18, 20)):
        assert not bits(t0[rows, 0]).any()           # +0.0, not -0.0
        assert np.isfinite(t0[rows, 1]).all() and t0[rows, 1].all()
    other = np.ones(n, dtype=bool)
    other[10:12] = other[18:20] = False
    assert np.array_equal(bits(t0[other]), bits(t1[other])) and np.isfinite(t0).all()
    # theta = 0.7 on the changed blocks: ordinary solves
    for rows, blk in ((slice(10, 12), np.zeros((2, 2))), (slice(18, 20), np.ones((2, 2)))):
        assert np.abs((0.7 * np.eye(2) - blk) @ t0[rows, 1] - r0[rows, 1]).max() < 1e-13


# ---- 3. b = 1 equals scalar DPR bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gev", [False, True], ids=["standard", "generalized"])
def test_block_size_one_is_scalar_dpr_bit_for_bit(gev):
    n, lowest = 300, 4
    a, bm = I.block_matrix(n, 1, 2, gev)
    with fd.CEngine(n=n, max_cols=66, gev=gev) as e:
        set_bsr(e, OP_A, I.bsr_of(a, 1))
        if gev:
            set_bsr(e, OP_B, I.bsr_of(bm, 1))
        for m in (5, 33):
            v, w, bv, theta = panels(n, m, m, gev)
            if not gev:
                theta[0] = a[7, 7]                       # an exactly zero denominator in row 7 of column 0
            _, t_dpr = correction(e, m, v, w, bv, theta, METHOD_DPR)
            _, t_blk = correction(e, m, v, w, bv, theta, METHOD_BDPR)
            assert np.array_equal(bits(t_dpr), bits(t_blk)), (gev, m)
            if not gev:
                assert t_blk[7, 0] == 0.0
    with fd.DavidsonEngine(n, lowest, gev=gev) as eng:
        eng.set_block_sparse(1, *I.bsr_of(a, 1))
        if gev:
            eng.set_block_sparse(2, *I.bsr_of(bm, 1))
        lam_d, _, it_d = eng.solve("DPR", 300, 1e-8, want_vectors=False)
        lam_b, _, it_b = eng.solve("BDPR", 300, 1e-8, want_vectors=False)
    assert it_d == it_b <= 300 and np.array_equal(bits(lam_d), bits(lam_b)), (it_d, it_b, lam_d - lam_b)


# ---- 4. refresh -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,gev", [(4, False), (7, True)])
def test_new_values_reach_the_diagonal_blocks(b, gev):
    n, m = b * -(-300 // b), 16
    a1, b1 = I.block_matrix(n, b, 1, gev)
    a2, b2 = I.block_matrix(n, b, 2, gev)          # the same pattern, other numbers
    v, w, bv, theta = panels(n, m, 9, gev)
    arr1, arr2 = I.bsr_of(a1, b, split=3), I.bsr_of(a2, b, split=3)
    assert np.array_equal(arr1[0], arr2[0]) and np.array_equal(arr1[1], arr2[1])
    with fd.CEngine(n=n, max_cols=2 * m, gev=gev) as e:
        e.keep_value_map(OP_A)
        set_bsr(e, OP_A, arr1)
        if gev:
            e.keep_value_map(OP_B)
            set_bsr(e, OP_B, I.bsr_of(b1, b))
        _, t1 = correction(e, m, v, w, bv, theta, METHOD_BDPR)
        e.update_operator_values(OP_A, arr2[2])
        if gev:
            e.update_operator_values(OP_B, I.bsr_of(b2, b)[2])
        _, t2 = correction(e, m, v, w, bv, theta, METHOD_BDPR)
    with fd.CEngine(n=n, max_cols=2 * m, gev=gev) as e:
        set_bsr(e, OP_A, arr2)
        if gev:
            set_bsr(e, OP_B, I.bsr_of(b2, b))
        _, fresh = correction(e, m, v, w, bv, theta, METHOD_BDPR)
    assert not np.array_equal(bits(t1), bits(t2))
    assert np.array_equal(bits(t2), bits(fresh))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def csr_of(a):
    rows, cols = np.nonzero(a)
    indptr = np.searchsorted(rows, np.arange(a.shape[0] + 1)).astype(np.int64)
    return indptr, cols.astype(np.int32), a[rows, cols]


@pytest.mark.parametrize("case", ["a_csr", "a_dense", "b_other_block", "b_csr"])
def test_operators_the_method_does_not_serve_are_refused(case):
    n, b, m = 240, 4, 5
    a, bm = I.block_matrix(n, b, 1, gev=True)
    gev = case.startswith("b_")
    v, w, bv, theta = panels(n, m, 4, gev)
    with fd.CEngine(n=n, max_cols=16, gev=gev) as e:
        if case == "a_csr":
            e.set_operator_csr(OP_A, *csr_of(a))
            want = "operator A is a CSR matrix"
        elif case == "a_dense":
            e.set_dense_host(OP_A, np.asfortranarray(a))
            want = "operator A is a dense matrix"
        else:
            set_bsr(e, OP_A, I.bsr_of(a, b))
            if case == "b_other_block":
                set_bsr(e, OP_B, I.bsr_of(bm, 2))
                want = "operator B has block size 2, operator A has 4"
            else:
                e.set_operator_csr(OP_B, *csr_of(bm))
                want = "operator B is a CSR matrix"
        mark = np.full((n, m), 3.25)
        e.panel_put(PANEL_V, m, mark)
        e.panel_put(PANEL_R, 0, mark)
        with pytest.raises(DavidsonHipError, match=re.escape(want)) as exc:
            correction(e, m, v, w, bv, theta, METHOD_BDPR)
        assert "BDPR" in str(exc.value)
        assert np.array_equal(bits(e.panel_get(PANEL_V, 0, m)), bits(v))
        assert np.array_equal(e.panel_get(PANEL_V, m, m), mark) and np.array_equal(e.panel_get(PANEL_R, 0, m), mark)
        # the engine stays usable: scalar DPR on the same panels
        _, t = correction(e, m, v, w, bv, theta, METHOD_DPR)
        assert np.isfinite(t).all()


def three_ranks(n, max_cols, work, gev=False):
    """work(engine, rank) on three engines of one in-process group, one thread each; returns the results"""
    nranks = 3
    engs = [fd.CEngine(n=n, max_cols=max_cols, gev=gev, rank=r, nranks=nranks) for r in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def run(r):
        try:
            out[r] = work(engs[r], r)
        except Exception as exc:      # noqa: BLE001
            err[r] = exc
        finally:
            fd.hip_lib().dav_local_group_yield(engs[r].h)

    th = [threading.Thread(target=run, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join() for t in th]
    for e in engs:
        e.close()
    assert all(x is None for x in err), err
    return out


def test_a_block_that_straddles_two_ranks_is_refused():
    n, b, m = 240, 3, 5                             # 80 rows per rank: not a multiple of 3
    a, _ = I.block_matrix(n, b, 1)
    arrays = I.bsr_of(a, b)
    v, w, _, theta = panels(n, m, 4, False)

    def work(e, r):
        set_bsr(e, OP_A, arrays)
        with pytest.raises(DavidsonHipError, match="does not divide the 80 rows") as exc:
            correction(e, m, v, w, None, theta, METHOD_BDPR)
        assert "operator A" in str(exc.value) and "straddle" in str(exc.value)
        return e.panel_get(PANEL_V, 0, m)

    for got in three_ranks(n, 16, work):
        assert np.array_equal(bits(got), bits(v))


# ---- 6. three ranks against one ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [4, 5, 16])
def test_three_ranks_match_one_rank(b):
    n, m, lowest = 240, 16, 4
    a, _ = I.block_matrix(n, b, 1)
    arrays = I.bsr_of(a, b)
    v, w, _, theta = panels(n, m, b, False)
    with fd.CEngine(n=n, max_cols=2 * m) as e:
        set_bsr(e, OP_A, arrays)
        r1, t1 = correction(e, m, v, w, None, theta, METHOD_BDPR)

    def work(e, r):
        set_bsr(e, OP_A, arrays)
        return correction(e, m, v, w, None, theta, METHOD_BDPR)

    for r3, t3 in three_ranks(n, 2 * m, work):
        assert np.array_equal(bits(r3), bits(r1)) and np.array_equal(bits(t3), bits(t1))

    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_block_sparse(1, *arrays)
        lam1, _, it1 = eng.solve("BDPR", 300, 1e-8, want_vectors=False)
    nranks = 3
    engs = [fd.DavidsonEngine(n, lowest, rank=rk, nranks=nranks) for rk in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.c.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def solve(rk):
        try:
            engs[rk].set_block_sparse(1, *arrays)
            out[rk] = engs[rk].solve("BDPR", 300, 1e-8, want_vectors=False)
        except Exception as exc:      # noqa: BLE001
            err[rk] = exc
        finally:
            fd.hip_lib().dav_local_group_yield(engs[rk].c.h)

    th = [threading.Thread(target=solve, args=(rk,)) for rk in range(nranks)]
    [t.start() for t in th]
    [t.join() for t in th]
    for e in engs:
        e.close()
    assert all(x is None for x in err), err
    assert it1 <= 300
    for lam, _, it in out:
        assert it == it1 and np.abs(lam - lam1).max() < 1e-10


# ---- 7. solves --------------------------------------------------------------------------------------------------------------------------
SOLVES = [(240, 4, 1, False), (256, 16, 1, False), (240, 8, 2, False), (240, 4, 1, True)]


def check_pairs(a, bm, lam, vec, ref):
    res = a @ vec - (vec if bm is None else bm @ vec) * lam[None, :]
    assert np.linalg.norm(res, axis=0).max() < 1e-8
    assert np.abs(lam - ref).max() < 1e-8


@pytest.mark.parametrize("n,b,seed,gev", SOLVES)
def test_solves_converge_in_fewer_iterations_than_scalar_dpr(n, b, seed, gev):
    lowest = 4
    a, bm = I.block_matrix(n, b, seed, gev)
    ref = eigh_lowest(a, bm, lowest)
    with fd.DavidsonEngine(n, lowest, gev=gev) as eng:
        eng.set_block_sparse(1, *I.bsr_of(a, b))
        if gev:
            eng.set_block_sparse(2, *I.bsr_of(bm, b))
        lam, vec, it = eng.solve("BDPR", 300, 1e-8)
        lam_d, vec_d, it_d = eng.solve("DPR", 300, 1e-8)
    assert it <= 300 and it_d <= 300
    check_pairs(a, bm, lam, vec, ref)
    check_pairs(a, bm, lam_d, vec_d, ref)
    it_dpr_restated, it_restated = I.TABLE[(n, b, gev, seed)]
    print(f"n={n} b={b} seed={seed} gev={gev}: BDPR {it} iterations (restatement {it_restated}), DPR {it_d} (restatement {it_dpr_restated})")
    # (side by side with the restatement's counts above; the elimination is not bitwise numpy's, so equality is not required)
    assert 3 * it <= 2 * it_d, (it, it_d, it_restated, it_dpr_restated)


def test_the_one_call_front_end_solves_with_bdpr():
    n, b, lowest = 240, 4, 4
    a, bm = I.block_matrix(n, b, 1, True)
    lam, vec, it = fd.solver.generalized_eigensolver_bsr(*I.bsr_of(a, b), lowest, "BDPR", 300, 1e-8, second=I.bsr_of(bm, b))
    assert it <= 300
    check_pairs(a, bm, lam, vec, eigh_lowest(a, bm, lowest))
    lam, vec, it = fd.solver.generalized_eigensolver_bsr(*I.bsr_of(a, b, lower=True), lowest, "BDPR", 300, 1e-8, lower=True)
    assert it <= 300
    check_pairs(a, None, lam, vec, eigh_lowest(a, None, lowest))


@pytest.mark.parametrize("option", ["unconverged", "locking", "device_rr"])
def test_policies_and_device_rayleigh_ritz_reach_the_same_eigenvalues(option):
    n, b, lowest = 240, 4, 4
    a, _ = I.block_matrix(n, b, 1)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_block_sparse(1, *I.bsr_of(a, b))
        if option == "device_rr":
            eng.set_device_rr(True)
        else:
            eng.set_correction_policy(option)
        lam, vec, it = eng.solve("BDPR", 300, 1e-8)
    assert it <= 300
    check_pairs(a, None, lam, vec, eigh_lowest(a, None, lowest))


# ---- 8. the Fortran program -------------------------------------------------------------------------------------------------------------
def fortran_matrices(n=240, b=4):
    """the matrices tests/fortran/prog_bdpr.f90 builds, from the same integer formulas"""
    nb = n // b
    a, bm = np.zeros((n, n)), np.eye(n)
    for bi in range(1, nb + 1):
        for r in range(1, b + 1):
            for c in range(1, b + 1):
                i, j = (bi - 1) * b + r - 1, (bi - 1) * b + c - 1
                a[i, j] = ((17 * bi + 5 * (r + c) + 3 * r * c) % 11) / 11.0 - 0.5
                bm[i, j] += 0.1 * (((7 * bi + 2 * (r + c) + r * c) % 13) / 13.0 - 0.5)
                if r == c:
                    a[i, j] += (r - 1) * 1.0 + 0.01 * (bi - 1)
                if bi > 1:
                    h = 0.05 * (((5 * bi + 3 * r + 7 * c) % 17) / 17.0 - 0.5)
                    a[i, j - b] = h
                    a[j - b, i] = h
                    s = 0.01 * (((3 * bi + 5 * r + 2 * c) % 19) / 19.0 - 0.5)
                    bm[i, j - b] = s
                    bm[j - b, i] = s
    return a, bm


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang not available")
def test_fortran_program_solves_with_bdpr(tmp_path):
    from test_fortran_programs import SRC, _run, compile_link
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    exe = compile_link([os.path.join(SRC, "prog_bdpr.f90")], os.path.join(bindir, "prog_bdpr"), tmp_path)
    rc, out = _run(exe)
    assert rc == 0, out
    a, bm = fortran_matrices()
    it_std, it_gen, it_dpr = [int(x) for x in re.search(r"ITERS\s+(\d+)\s+(\d+)\s+(\d+)", out).groups()]
    assert it_std <= 300 and it_gen <= 300 and it_std < it_dpr
    for label, second in (("EVALS_STD", None), ("EVALS_GEN", bm)):
        ev = np.array([float(x) for x in re.search(label + r"(.*)", out).group(1).split()])
        assert np.abs(ev - eigh_lowest(a, second, 4)).max() < 1e-8, label
    checks = re.findall(r"CHECK (\S+) ([TF])", out)
    assert len(checks) == 8 and all(v == "T" for _, v in checks), out
