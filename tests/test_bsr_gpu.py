"""Block-sparse (BSR) operators on the GPU (dav_set_operator_bsr): the block product of the engine's matrix-core kernel
(fortran_davidson_amd/csrc/k_bsrmm.hip) against a host product over block sizes, storages, bases, layouts and widths, its bitwise
reproducibility over repetitions and rank counts (block rows that straddle two slabs included), solves against the oracle, BSR against
CSR and dense storage of the same matrix, three ranks, a full-order problem, the validation errors, and the Fortran program that solves a
bsr_matrix through the generic."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import BSR_COL_MAJOR, BSR_ROW_MAJOR, OP_A, PANEL_V, PANEL_W, DavidsonHipError
from oracle import davidson_oracle as O

pytestmark = pytest.mark.gpu


# ---- BSR inputs, built with numpy ---------------------------------------------------------------------------------------------------
def blocks_to_bsr(nb, bi, bj, blk):
    """BSR arrays of block triples in the given order within each block row (stable): duplicates and their order are kept"""
    order = np.argsort(bi, kind="stable")
    bi, bj, blk = bi[order], bj[order], blk[order]
    indptr = np.searchsorted(bi, np.arange(nb + 1)).astype(np.int64)
    return indptr, bj.astype(np.int32), np.ascontiguousarray(blk, dtype=np.float64)


def symmetric_blocks(nb, b, rng, kind="random", per_row=3):
    """(block rows, block columns, blocks) of a symmetric block matrix, every nonzero block listed: symmetric diagonal blocks (dominant),
    random off-diagonal blocks mirrored; "random" also leaves some block rows empty and splits some blocks into two terms;
    "arrowhead" couples block row 0 with every block column"""
    if kind == "arrowhead":
        off_i = np.arange(1, nb)
        off_j = np.zeros(nb - 1, dtype=np.int64)
    else:
        off_i = np.repeat(np.arange(nb), per_row)
        off_j = rng.integers(0, nb, off_i.size)
        keep = off_i != off_j
        off_i, off_j = off_i[keep], off_j[keep]
    w = rng.uniform(-1e-2, 1e-2, (off_i.size, b, b))
    d = rng.uniform(-1e-2, 1e-2, (nb, b, b))
    d = d + d.transpose(0, 2, 1)
    d += np.eye(b)[None] * (1.0 + np.arange(nb * b, dtype=np.float64).reshape(nb, b))[:, :, None]
    bi = np.concatenate([np.arange(nb), off_i, off_j])
    bj = np.concatenate([np.arange(nb), off_j, off_i])
    blk = np.concatenate([d, w, w.transpose(0, 2, 1)])
    if kind == "random":
        dead = (bi % 7 == 3) | (bj % 7 == 3)                     # empty block rows (and block columns)
        bi, bj, blk = bi[~dead], bj[~dead], blk[~dead]
        sel = (np.minimum(bi, bj) + np.maximum(bi, bj)) % 4 == 1  # duplicates: a block and its mirror split alike
        bi, bj = np.concatenate([bi, bi[sel]]), np.concatenate([bj, bj[sel]])
        blk = np.concatenate([np.where(sel[:, None, None], 0.75 * blk, blk), 0.25 * blk[sel]])
    return bi, bj, blk


def bsr_input(nb, bi, bj, blk, lower, layout, rng):
    """what the caller passes: every block or only J <= I, blocks shuffled within their block rows, in the given layout"""
    if lower:
        sel = bj <= bi
        bi, bj, blk = bi[sel], bj[sel], blk[sel]
    perm = rng.permutation(bi.size)
    rp, ci, vv = blocks_to_bsr(nb, bi[perm], bj[perm], blk[perm])
    if layout == BSR_COL_MAJOR:
        vv = np.ascontiguousarray(vv.transpose(0, 2, 1))
    return rp, ci, vv


def host_product(n, b, bi, bj, blk, x):
    """(A X in extended precision, |A| |X|) from the full block triples"""
    k = x.shape[1]
    xs = x.reshape(n // b, b, k)
    t = np.einsum("pmq,pqc->pmc", blk.astype(np.longdouble), xs[bj].astype(np.longdouble))
    y = np.zeros((n // b, b, k), dtype=np.longdouble)
    np.add.at(y, bi, t)
    tb = np.einsum("pmq,pqc->pmc", np.abs(blk), np.abs(xs[bj]))
    bound = np.zeros((n // b, b, k))
    np.add.at(bound, bi, tb)
    return y.reshape(n, k), bound.reshape(n, k)


def dense_of(n, b, bi, bj, blk):
    a = np.zeros((n // b, b, n // b, b))
    np.add.at(a, (bi, slice(None), bj), blk)            # a[bi[p], :, bj[p], :] += blk[p]
    return np.asfortranarray(a.reshape(n, n))


def bsr_of_dense(a, b, lower=False):
    """BSR arrays of the nonzero blocks of a dense matrix (block columns <= block rows only, lower=True)"""
    n = a.shape[0]
    nb = n // b
    t = a.reshape(nb, b, nb, b).transpose(0, 2, 1, 3)
    bi, bj = np.nonzero(np.abs(t).sum(axis=(2, 3)) > 0)
    if lower:
        sel = bj <= bi
        bi, bj = bi[sel], bj[sel]
    return blocks_to_bsr(nb, bi, bj, t[bi, bj])


def put_apply_get(e, x, k):
    e.panel_put(PANEL_V, 0, x[:, :k])
    e.apply(OP_A, PANEL_V, 0, k, PANEL_W, 0)
    return e.panel_get(PANEL_W, 0, k)


KS = (1, 7, 16, 33, 64)
BS = (1, 2, 3, 4, 5, 8, 12, 16)
STORAGES = [(False, 0, BSR_ROW_MAJOR), (True, 1, BSR_COL_MAJOR), (False, 1, BSR_COL_MAJOR), (True, 0, BSR_ROW_MAJOR)]


# ---- 1. apply parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", BS)
def test_apply_matches_the_host_product(b):
    nb = 61
    n = nb * b
    rng = np.random.default_rng(b)
    bi, bj, blk = symmetric_blocks(nb, b, rng)
    x = rng.standard_normal((n, max(KS)))
    refs = {k: host_product(n, b, bi, bj, blk, x[:, :k]) for k in KS}
    diag = np.zeros(n)
    for I, J, B in zip(bi, bj, blk):
        if I == J:
            diag[I * b:(I + 1) * b] += np.diag(B)
    with fd.CEngine(n=n, max_cols=max(KS)) as e:
        for lower, base, layout in STORAGES:
            rp, ci, vv = bsr_input(nb, bi, bj, blk, lower, layout, rng)
            e.set_operator_bsr(OP_A, rp + base, ci + base, vv, base=base, lower=lower, layout=layout)
            assert np.allclose(e.get_diagonal(OP_A), diag, rtol=1e-15, atol=0)
            for k in KS:
                y = put_apply_get(e, x, k)
                ref, bound = refs[k]
                err = np.abs(y.astype(np.longdouble) - ref).astype(np.float64)
                assert (err <= 1e-13 * bound + 1e-300).all(), (b, lower, base, layout, k, float(err.max()))


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------------
def three_rank_apply(n, rp, ci, vv, x, k):
    nranks = 3
    engs = [fd.CEngine(n=n, max_cols=64, rank=r, nranks=nranks) for r in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def work(r):
        try:
            engs[r].set_operator_bsr(OP_A, rp, ci, vv)
            out[r] = put_apply_get(engs[r], x, k)
        except Exception as exc:      # noqa: BLE001
            err[r] = exc
        finally:
            fd.hip_lib().dav_local_group_yield(engs[r].h)

    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join() for t in th]
    slabs = [engs[r].local_rows() for r in range(nranks)]
    for e in engs:
        e.close()
    assert all(x is None for x in err), err
    return out, slabs


# N = 1050 on three ranks: slabs of 352 rows, so block rows of b = 3, 5, 6, 7 straddle two ranks; the arrowhead's first block row holds
# all 350 block columns (three chunks)
@pytest.mark.parametrize("b,n,kind", [(3, 1050, "random"), (5, 1050, "random"), (6, 1050, "random"), (7, 1050, "random"),
                                      (12, 1056, "random"), (3, 1050, "arrowhead")])
def test_applies_are_bitwise_reproducible_over_repetitions_and_ranks(b, n, kind):
    rng = np.random.default_rng(100 + b)
    nb = n // b
    bi, bj, blk = symmetric_blocks(nb, b, rng, kind)
    rp, ci, vv = bsr_input(nb, bi, bj, blk, False, BSR_ROW_MAJOR, rng)
    x = rng.standard_normal((n, 64))
    with fd.CEngine(n=n, max_cols=64) as e:
        e.set_operator_bsr(OP_A, rp, ci, vv)
        one = {k: put_apply_get(e, x, k) for k in (16, 40)}
        for k in (16, 40):
            assert np.array_equal(put_apply_get(e, x, k), one[k])
        ref, bound = host_product(n, b, bi, bj, blk, x[:, :16])
        assert (np.abs(one[16] - ref.astype(np.float64)) <= 1e-13 * bound + 1e-300).all()
    for k in (16, 40):
        out, slabs = three_rank_apply(n, rp, ci, vv, x, k)
        for r, (r0, nl) in enumerate(slabs):
            assert np.array_equal(out[r][r0:r0 + nl], one[k][r0:r0 + nl]), (b, kind, k, r)


# ---- 3. solves against the oracle -------------------------------------------------------------------------------------------------
def banded(n, d0, dstep, eps):
    """d0 + dstep * i on the diagonal, eps and eps / 2 on the first two off-diagonals"""
    a = np.diag(d0 + dstep * np.arange(n, dtype=np.float64))
    for off, w in ((1, eps), (2, 0.5 * eps)):
        a += w * (np.eye(n, k=off) + np.eye(n, k=-off))
    return np.asfortranarray(a)


def block_dd(n, b, seed):
    """symmetric, diagonally dominant block matrix (dense): diagonal i + 1, three random coupling blocks per block row"""
    nb = n // b
    bi, bj, blk = symmetric_blocks(nb, b, np.random.default_rng(seed), "plain")
    return dense_of(n, b, bi, bj, blk)


@pytest.mark.parametrize("gev,method,n,b,lowest", [(False, "DPR", 2000, 8, 4), (False, "GJD", 1500, 5, 4), (True, "DPR", 2400, 16, 3),
                                                   (True, "GJD", 1200, 4, 3)])
def test_solves_match_the_oracle(gev, method, n, b, lowest):
    a = block_dd(n, b, 11) if (method, gev) == ("DPR", False) else banded(n, 1.0, 1.0, 0.3)
    bm = banded(n, 1.0, 0.0, 0.05) if gev else None
    lam_o, _, it_o = O.generalized_eigensolver_dense(a, lowest, method, 200, 1e-8, None, bm)
    second = bsr_of_dense(bm, b) if gev else None
    lam, vec, it = fd.generalized_eigensolver_bsr(*bsr_of_dense(a, b), lowest, method, 200, 1e-8, second=second)
    assert it == it_o
    assert np.abs(lam - lam_o).max() < 1e-9
    bx = vec if bm is None else bm @ vec
    assert np.linalg.norm(a @ vec - bx * lam[None, :], axis=0).max() < 1e-8


def test_locking_policy_on_a_bsr_operator():
    n, b, lowest = 1500, 6, 4
    a = block_dd(n, b, 21)
    lam_o, _, it_o = O.generalized_eigensolver_dense_locking(a, lowest, "DPR", 300, 1e-8, None)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_block_sparse(1, *bsr_of_dense(a, b, lower=True), lower=True)
        eng.set_correction_policy("locking")
        lam, vec, it = eng.solve("DPR", 300, 1e-8)
    assert it == it_o
    assert np.abs(lam - lam_o).max() < 1e-9
    assert np.linalg.norm(a @ vec - vec * lam[None, :], axis=0).max() < 1e-8


# ---- 4. BSR, CSR and dense storage of one matrix -----------------------------------------------------------------------------------
def test_bsr_csr_and_dense_storage_of_the_same_matrix_agree():
    n, b, lowest = 20000, 8, 8
    nb = n // b
    bi, bj, blk = symmetric_blocks(nb, b, np.random.default_rng(31), "plain", per_row=6)
    results = []
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_block_sparse(1, *blocks_to_bsr(nb, bi, bj, blk))
        results.append(eng.solve("DPR", 200, 1e-8, want_vectors=False))
    rows = (bi[:, None, None] * b + np.arange(b)[None, :, None] + 0 * np.arange(b)[None, None, :]).ravel()
    cols = (bj[:, None, None] * b + 0 * np.arange(b)[None, :, None] + np.arange(b)[None, None, :]).ravel()
    order = np.argsort(rows, kind="stable")
    indptr = np.searchsorted(rows[order], np.arange(n + 1)).astype(np.int64)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_sparse(1, indptr, cols[order].astype(np.int32), blk.ravel()[order])
        results.append(eng.solve("DPR", 200, 1e-8, want_vectors=False))
    a = dense_of(n, b, bi, bj, blk)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_dense(1, a)
        results.append(eng.solve("DPR", 200, 1e-8, want_vectors=False))
    del a
    (lam_b, _, it_b), (lam_c, _, it_c), (lam_d, _, it_d) = results
    assert it_b == it_c == it_d
    assert np.abs(lam_b - lam_c).max() < 1e-10 and np.abs(lam_b - lam_d).max() < 1e-10


# ---- 5. three ranks -----------------------------------------------------------------------------------------------------------------
def test_three_rank_solve_matches_one_rank():
    n, b, lowest, nranks = 2100, 6, 4, 3              # slabs of 704 rows: block rows straddle the ranks
    a = block_dd(n, b, 41)
    bsr = bsr_of_dense(a, b)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_block_sparse(1, *bsr)
        lam1, _, it1 = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    engs = [fd.DavidsonEngine(n, lowest, rank=rk, nranks=nranks) for rk in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.c.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def work(rk):
        try:
            engs[rk].set_block_sparse(1, *bsr)
            out[rk] = engs[rk].solve("DPR", 200, 1e-8, want_vectors=False)
        except Exception as exc:      # noqa: BLE001
            err[rk] = exc
        finally:
            fd.hip_lib().dav_local_group_yield(engs[rk].c.h)

    th = [threading.Thread(target=work, args=(rk,)) for rk in range(nranks)]
    [t.start() for t in th]
    [t.join() for t in th]
    for e in engs:
        e.close()
    assert all(x is None for x in err), err
    for lam, _, it in out:
        assert it == it1 and np.abs(lam - lam1).max() < 1e-10


# ---- 6. full order --------------------------------------------------------------------------------------------------------------------
def test_a_million_rows_in_8x8_blocks():
    """N = 10^6, b = 8: a block band of half-width 4 (up to 9 blocks per block row, 0.58 GB of values)"""
    n, b, lowest, half = 1_000_000, 8, 8, 4
    nb = n // b
    I = np.arange(nb, dtype=np.int64)
    counts = np.minimum(I, half) + 1 + np.minimum(nb - 1 - I, half)
    indptr = np.zeros(nb + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    bi = np.repeat(I, counts)
    bj = np.maximum(I - half, 0)[bi] + (np.arange(indptr[-1], dtype=np.int64) - indptr[bi])
    r = bi[:, None, None] * b + np.arange(b)[None, :, None]
    c = bj[:, None, None] * b + np.arange(b)[None, None, :]
    d = np.abs(r - c)
    vals = np.where(d == 0, 1.0 + r.astype(np.float64), 1e-2 / (1.0 + d))
    del r, c, d
    lam, vec, it = fd.generalized_eigensolver_bsr(indptr, bj.astype(np.int32), vals, lowest, "DPR", 100, 1e-8)
    assert 0 < it < 100
    for j in range(lowest):
        xs = vec[:, j].reshape(nb, b)
        t = np.einsum("pmq,pq->pm", vals, xs[bj])
        av = np.add.reduceat(t, indptr[:-1], axis=0).ravel()
        assert np.linalg.norm(av - lam[j] * vec[:, j]) < 1e-8, j
    assert np.all(np.diff(lam) > 0)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------
def test_validation_errors_leave_the_engine_usable():
    n, b = 480, 4
    nb = n // b
    a = block_dd(n, b, 51)
    rp, ci, vv = bsr_of_dense(a, b)
    lrp, lci, lvv = bsr_of_dense(a, b, lower=True)
    bad_rp = rp.copy()
    bad_rp[50] = bad_rp[52]
    bad_ci = ci.copy()
    bad_ci[17] = nb
    lib = fd.hip_lib()

    def raw(e, bs, rp_, ci_, vv_, base=0, tri=0, layout=0):
        rc = lib.dav_set_operator_bsr(e.h, C.c_int(OP_A), C.c_int(bs), rp_.ctypes.data_as(C.POINTER(C.c_int64)),
                                      ci_.ctypes.data_as(C.POINTER(C.c_int32)), vv_.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(base),
                                      C.c_int(tri), C.c_int(layout))
        return rc, lib.dav_last_error().decode()

    with fd.CEngine(n=n, max_cols=16) as e:
        rp5, ci5, vv5 = bsr_of_dense(np.eye(475), 5)
        cases = [(lambda: raw(e, 0, rp, ci, vv), "block_size = 0 must lie in 1..16"),
                 (lambda: raw(e, 17, rp, ci, vv), "block_size = 17 must lie in 1..16"),
                 (lambda: raw(e, 7, rp5, ci5, vv5), "is not a multiple of block_size = 7"),
                 (lambda: raw(e, b, bad_rp, ci, vv), "block_row_ptr decreases at block row 50"),
                 (lambda: raw(e, b, rp, bad_ci, vv), f"block column {nb} out of range"),
                 (lambda: raw(e, b, rp, ci, vv, tri=1), "above the diagonal"),
                 (lambda: raw(e, b, rp, ci, vv, layout=2), "block_layout must be"),
                 (lambda: raw(e, b, rp + 1, ci + 1, vv), "must equal the index base 0")]
        for call, msg in cases:
            rc, err = call()
            assert rc != 0 and msg in err, (msg, err)
            with pytest.raises(DavidsonHipError, match="operator not set"):
                e.apply(OP_A, PANEL_V, 0, 1, PANEL_W, 0)
        with pytest.raises(DavidsonHipError, match="above the diagonal"):
            e.set_operator_bsr(OP_A, rp, ci, vv, lower=True)
        e.set_operator_bsr(OP_A, lrp, lci, np.ascontiguousarray(lvv.transpose(0, 2, 1)), lower=True, layout=BSR_COL_MAJOR)
        idx = e.init_basis(4)
        w = e.panel_get(PANEL_W, 0, 4)
        assert np.allclose(w, a[:, idx - 1], rtol=0, atol=1e-15)
        x = np.random.default_rng(1).standard_normal((n, 8))
        assert np.abs(put_apply_get(e, x, 8) - a @ x).max() < 1e-12
    lam_o, _, it_o = O.generalized_eigensolver_dense(a, 3, "DPR", 200, 1e-8, None)
    with fd.DavidsonEngine(n, 3) as eng:
        eng.set_block_sparse(1, rp, ci, vv)
        lam, _, it = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    assert it == it_o and np.abs(lam - lam_o).max() < 1e-9


# ---- 8. the Fortran program -------------------------------------------------------------------------------------------------------
def test_bsr_fortran_program_matches_the_oracle(tmp_path):
    from test_fortran_programs import SRC, _run, compile_link
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    exe = compile_link([os.path.join(SRC, "prog_bsr.f90")], os.path.join(bindir, "prog_bsr"), tmp_path)
    rc, out = _run(exe)
    assert rc == 0, out
    checks = re.findall(r"CHECK (\S+) ([TF])", out)
    assert len(checks) == 14 and all(v == "T" for _, v in checks), out
    n, lowest = 1200, 4
    a = banded(n, 1.0, 1.0, 0.3)
    b = banded(n, 1.0, 0.0, 0.05)
    iters = [int(x) for x in re.search(r"ITERS\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", out).groups()]
    for label, method, bb, it in (("EVALS_DPR", "DPR", None, iters[0]), ("EVALS_GJD", "GJD", None, iters[1]), ("EVALS_GEN", "DPR", b, iters[2])):
        lam_o, _, it_o = O.generalized_eigensolver_dense(a, lowest, method, 1000, 1e-8, 10 * lowest, bb)
        ev = np.array([float(x) for x in re.search(label + r"(.*)", out).group(1).split()])
        assert np.abs(ev - lam_o).max() < 1e-9, label
        assert it == it_o, label
