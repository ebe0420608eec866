"""Sparse (CSR) operators on the GPU (dav_set_operator_csr, ABI 109): the block product of the engine's own CSR kernel
(fortran_davidson_amd/csrc/k_spmm.hip) against a host product, its bitwise reproducibility over repetitions and rank counts, solves
against the oracle on the densified matrix, CSR against the engine's dense path, three ranks, a full-order problem no dense storage could
hold, the validation errors, and the Fortran program that solves a csr_matrix through the generic."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import OP_A, PANEL_V, PANEL_W, DavidsonHipError
from oracle import davidson_oracle as O

pytestmark = pytest.mark.gpu


# ---- CSR inputs, built with numpy ---------------------------------------------------------------------------------------------------
def coo_to_csr(n, rows, cols, vals):
    """CSR of COO triples in the given order within each row (stable by row): duplicates and their order are kept"""
    order = np.argsort(rows, kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order]
    indptr = np.searchsorted(rows, np.arange(n + 1)).astype(np.int64)
    return indptr, cols.astype(np.int32), vals.astype(np.float64)


def symmetric_coo(n, kind, rng):
    """(rows, cols, vals) of a symmetric matrix of the class `kind`, every nonzero listed (duplicates where the class has them)"""
    if kind == "banded":
        off = [(d, 0.1 / d) for d in range(1, 4)]
        r = [np.arange(n)]; c = [np.arange(n)]; v = [1.0 + np.arange(n, dtype=np.float64)]
        for d, w in off:
            i = np.arange(n - d)
            r += [i, i + d]; c += [i + d, i]; v += [np.full(n - d, w)] * 2
        return np.concatenate(r), np.concatenate(c), np.concatenate(v)
    if kind == "arrowhead":                      # first row and column hold all n entries
        i = np.arange(1, n)
        w = rng.uniform(-1e-3, 1e-3, n - 1)
        return (np.concatenate([[0], np.arange(1, n), np.zeros(n - 1, int), i]), np.concatenate([[0], np.arange(1, n), i, np.zeros(n - 1, int)]),
                np.concatenate([[1.0], 2.0 + np.arange(1, n), w, w]))
    # uniformly random columns, 12 per row (symmetrised), then the class's particularity
    i = np.repeat(np.arange(n), 6)
    j = rng.integers(0, n, i.size)
    keep = i != j
    i, j = i[keep], j[keep]
    w = rng.uniform(-1e-3, 1e-3, i.size)
    r, c, v = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([w, w])
    d = np.arange(n)
    dv = 1.0 + d.astype(np.float64)
    if kind == "missing_diagonal":
        sel = d % 7 != 3
        d, dv = d[sel], dv[sel]
    r, c, v = np.concatenate([r, d]), np.concatenate([c, d]), np.concatenate([v, dv])
    if kind == "empty_rows":                     # rows (and their columns) without any entry
        dead = (r % 11 == 5) | (c % 11 == 5)
        r, c, v = r[~dead], c[~dead], v[~dead]
    if kind == "duplicates":                     # every 5th entry split into two terms (both halves of a symmetric pair alike)
        sel = (np.minimum(r, c) + np.maximum(r, c)) % 5 == 0
        r, c, v = np.concatenate([r, r[sel]]), np.concatenate([c, c[sel]]), np.concatenate([np.where(sel, 0.75 * v, v), 0.25 * v[sel]])
    return r, c, v


def csr_input(n, rows, cols, vals, lower, rng):
    """the CSR arrays the caller passes: every nonzero, or only j <= i; entries shuffled within their rows"""
    if lower:
        sel = cols <= rows
        rows, cols, vals = rows[sel], cols[sel], vals[sel]
    perm = rng.permutation(rows.size)
    return coo_to_csr(n, rows[perm], cols[perm], vals[perm])


def host_product(n, rows, cols, vals, x):
    """(A X in extended precision, |A| |X|) from the symmetric COO triples"""
    y = np.zeros((n, x.shape[1]), dtype=np.longdouble)
    np.add.at(y, rows, vals[:, None].astype(np.longdouble) * x[cols].astype(np.longdouble))
    b = np.zeros((n, x.shape[1]))
    np.add.at(b, rows, np.abs(vals)[:, None] * np.abs(x[cols]))
    return y, b


def dense_of(n, rows, cols, vals):
    a = np.zeros((n, n), order="F")
    np.add.at(a, (rows, cols), vals)
    return a


def put_apply_get(e, x, k):
    e.panel_put(PANEL_V, 0, x[:, :k])
    e.apply(OP_A, PANEL_V, 0, k, PANEL_W, 0)
    return e.panel_get(PANEL_W, 0, k)


KS = (1, 7, 16, 17, 33, 64, 96)
CLASSES = ("banded", "random", "empty_rows", "missing_diagonal", "duplicates", "arrowhead")


# ---- 1. apply parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CLASSES)
@pytest.mark.parametrize("lower,base", [(False, 0), (True, 1)])
def test_apply_matches_the_host_product(kind, lower, base):
    n = 3001 if kind == "arrowhead" else 1003          # not multiples of 16; the arrowhead row is longer than one chunk (1024)
    rng = np.random.default_rng(CLASSES.index(kind) * 10 + lower)
    rows, cols, vals = symmetric_coo(n, kind, rng)
    rp, ci, vv = csr_input(n, rows, cols, vals, lower, rng)
    x = rng.standard_normal((n, max(KS)))
    with fd.CEngine(n=n, max_cols=max(KS)) as e:
        e.set_operator_csr(OP_A, rp + base, ci + base, vv, base=base, lower=lower)
        diag = np.zeros(n)
        np.add.at(diag, rows[rows == cols], vals[rows == cols])
        assert np.array_equal(e.get_diagonal(OP_A), diag)
        for k in KS:
            y = put_apply_get(e, x, k)
            ref, bound = host_product(n, rows, cols, vals, x[:, :k])
            err = np.abs(y.astype(np.longdouble) - ref).astype(np.float64)
            assert (err <= 1e-14 * bound + 1e-300).all(), (kind, k, float(err.max()))


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------------
def three_rank_apply(n, rp, ci, vv, x, k):
    nranks = 3
    engs = [fd.CEngine(n=n, max_cols=64, rank=r, nranks=nranks) for r in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def work(r):
        try:
            engs[r].set_operator_csr(OP_A, rp, ci, vv)
            out[r] = put_apply_get(engs[r], x, k)
        except Exception as exc:      # noqa: BLE001
            err[r] = exc
        finally:
            fd.hip_lib().dav_local_group_yield(engs[r].h)

    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join() for t in th]
    row0 = [engs[r].local_rows() for r in range(nranks)]
    for e in engs:
        e.close()
    assert all(x is None for x in err), err
    return out, row0


@pytest.mark.parametrize("kind", ["random", "arrowhead"])
def test_applies_are_bitwise_reproducible_over_repetitions_and_ranks(kind):
    n = 2999
    rng = np.random.default_rng(7)
    rows, cols, vals = symmetric_coo(n, kind, rng)                 # random columns couple every slab with every other
    rp, ci, vv = csr_input(n, rows, cols, vals, False, rng)
    x = rng.standard_normal((n, 64))
    with fd.CEngine(n=n, max_cols=64) as e:
        e.set_operator_csr(OP_A, rp, ci, vv)
        one = {k: put_apply_get(e, x, k) for k in (16, 40)}
        for k in (16, 40):
            assert np.array_equal(put_apply_get(e, x, k), one[k])
    for k in (16, 40):
        out, slabs = three_rank_apply(n, rp, ci, vv, x, k)
        for r, (r0, nl) in enumerate(slabs):
            assert np.array_equal(out[r][r0:r0 + nl], one[k][r0:r0 + nl]), (kind, k, r)


# ---- 3. solves against the oracle -------------------------------------------------------------------------------------------------
def sparse_dd(n, seed, diag=None, per_row=8, scale=1e-2):
    """symmetric, diagonally dominant: diagonal i + 1 (or `diag`), per_row random couplings per row of size `scale`"""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(n), per_row // 2)
    j = rng.integers(0, n, i.size)
    keep = i != j
    i, j = i[keep], j[keep]
    w = rng.uniform(0, scale, i.size)
    d = np.arange(n)
    dv = 1.0 + d.astype(np.float64) if diag is None else np.full(n, float(diag))
    return np.concatenate([i, j, d]), np.concatenate([j, i, d]), np.concatenate([w, w, dv])


def stencil_coo(n, d0, dstep, eps):
    """d0 + dstep * i on the diagonal, eps and eps / 2 on the first two off-diagonals (tests/test_device_operator_gpu.py's matrix)"""
    i = np.arange(n)
    r, c, v = [i], [i], [d0 + dstep * i.astype(np.float64)]
    for off, w in ((1, eps), (2, 0.5 * eps)):
        j = np.arange(n - off)
        r += [j, j + off]; c += [j + off, j]; v += [np.full(n - off, w)] * 2
    return np.concatenate(r), np.concatenate(c), np.concatenate(v)


# random couplings (DPR, standard) and the banded pencil of the device-operator tests (GJD, generalized)
@pytest.mark.parametrize("gev,method,n,lowest", [(False, "DPR", 2000, 4), (False, "GJD", 1500, 4), (True, "DPR", 2500, 3),
                                                 (True, "GJD", 1200, 3)])
def test_solves_match_the_oracle(gev, method, n, lowest):
    ra, ca, va = sparse_dd(n, 11) if (method, gev) == ("DPR", False) else stencil_coo(n, 1.0, 1.0, 0.3)
    a = dense_of(n, ra, ca, va)
    b = None
    second = None
    if gev:
        rb, cb, vb = stencil_coo(n, 1.0, 0.0, 0.05)
        b = dense_of(n, rb, cb, vb)
        second = coo_to_csr(n, rb, cb, vb)
    lam_o, _, it_o = O.generalized_eigensolver_dense(a, lowest, method, 200, 1e-8, None, b)
    lam, vec, it = fd.generalized_eigensolver_sparse(*coo_to_csr(n, ra, ca, va), lowest, method, 200, 1e-8, second=second)
    assert it == it_o
    assert np.abs(lam - lam_o).max() < 1e-9
    bx = vec if b is None else b @ vec
    assert np.linalg.norm(a @ vec - bx * lam[None, :], axis=0).max() < 1e-8


def test_locking_policy_on_a_csr_operator():
    n, lowest = 1500, 4
    r, c, v = sparse_dd(n, 21)
    a = dense_of(n, r, c, v)
    lam_o, _, it_o = O.generalized_eigensolver_dense_locking(a, lowest, "DPR", 300, 1e-8, None)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_sparse(1, *coo_to_csr(n, r, c, v))
        eng.set_correction_policy("locking")
        lam, vec, it = eng.solve("DPR", 300, 1e-8)
    assert it == it_o
    assert np.abs(lam - lam_o).max() < 1e-9
    assert np.linalg.norm(a @ vec - vec * lam[None, :], axis=0).max() < 1e-8


# ---- 4. CSR against the engine's own dense path --------------------------------------------------------------------------------------
def test_csr_and_dense_storage_of_the_same_matrix_agree():
    n, lowest = 20000, 8
    r, c, v = sparse_dd(n, 31, per_row=100)                       # density 0.005
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_sparse(1, *coo_to_csr(n, r, c, v), lower=False)
        lam_s, _, it_s = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    a = dense_of(n, r, c, v)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_dense(1, a)
        lam_d, _, it_d = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    del a
    assert it_s == it_d
    assert np.abs(lam_s - lam_d).max() < 1e-10


# ---- 5. three ranks -----------------------------------------------------------------------------------------------------------------
def test_three_rank_solve_matches_one_rank():
    n, lowest, nranks = 2999, 4, 3
    r, c, v = sparse_dd(n, 41)
    csr = coo_to_csr(n, r, c, v)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_sparse(1, *csr)
        lam1, _, it1 = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    engs = [fd.DavidsonEngine(n, lowest, rank=rk, nranks=nranks) for rk in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.c.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def work(rk):
        try:
            engs[rk].set_sparse(1, *csr)
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
def test_a_million_rows_no_dense_storage_could_hold():
    """N = 10^6, 65 nonzeros per row (a band of 32 on each side): 8 TB as a dense matrix, 0.8 GB in CSR"""
    n, lowest, half = 1_000_000, 8, 32
    counts = np.minimum(np.arange(n), half) + 1 + np.minimum(n - 1 - np.arange(n), half)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    rows = np.repeat(np.arange(n, dtype=np.int64), counts)
    first = np.maximum(np.arange(n, dtype=np.int64) - half, 0)
    cols = (first[rows] + (np.arange(indptr[-1], dtype=np.int64) - indptr[rows])).astype(np.int32)
    d = np.abs(cols - rows)
    vals = np.where(d == 0, 1.0 + rows.astype(np.float64), 1e-2 / (1.0 + d))
    del d
    lam, vec, it = fd.generalized_eigensolver_sparse(indptr, cols, vals, lowest, "DPR", 100, 1e-8)
    assert 0 < it < 100
    for j in range(lowest):
        av = np.add.reduceat(vals * vec[cols, j], indptr[:-1])
        assert np.linalg.norm(av - lam[j] * vec[:, j]) < 1e-8, j
    assert np.all(np.diff(lam) > 0)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------
def test_validation_errors_leave_the_engine_usable():
    n = 500
    rp, ci, vv = coo_to_csr(n, *sparse_dd(n, 51))
    lower_rp, lower_ci, lower_vv = csr_input(n, *sparse_dd(n, 51), True, np.random.default_rng(0))
    bad_rp = rp.copy()
    bad_rp[100] = bad_rp[102]
    bad_ci = ci.copy()
    bad_ci[17] = n
    neg_ci = ci.copy()
    neg_ci[3] = -1
    with fd.CEngine(n=n, max_cols=16) as e:
        cases = [((bad_rp, ci, vv), {}, "row_ptr decreases at row 100"),
                 ((rp, bad_ci, vv), {}, f"column index {n} out of range"),
                 ((rp, neg_ci, vv), {}, "column index -1 out of range"),
                 ((rp, ci, vv), {"lower": True}, "above the diagonal"),
                 ((rp + 1, ci + 1, vv), {}, "must equal the index base 0"),
                 ((rp, ci, vv), {"base": 2}, "index_base must be 0 or 1")]
        for args, kw, msg in cases:
            with pytest.raises(DavidsonHipError, match=re.escape(msg)):
                e.set_operator_csr(OP_A, *args, **kw)
            with pytest.raises(DavidsonHipError, match="operator not set"):
                e.apply(OP_A, PANEL_V, 0, 1, PANEL_W, 0)
        e.set_operator_csr(OP_A, lower_rp, lower_ci, lower_vv, lower=True)
        idx = e.init_basis(4)
        w = e.panel_get(PANEL_W, 0, 4)
        a = dense_of(n, *sparse_dd(n, 51))
        assert np.allclose(w, a[:, idx - 1], rtol=0, atol=1e-15)
        x = np.random.default_rng(1).standard_normal((n, 8))
        assert np.abs(put_apply_get(e, x, 8) - a @ x).max() < 1e-12


# ---- 8. the Fortran program -------------------------------------------------------------------------------------------------------
def test_sparse_fortran_program_matches_the_oracle(tmp_path):
    from test_fortran_programs import SRC, _run, compile_link
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    exe = compile_link([os.path.join(SRC, "prog_sparse.f90")], os.path.join(bindir, "prog_sparse"), tmp_path)
    rc, out = _run(exe)
    assert rc == 0, out
    checks = re.findall(r"CHECK (\S+) ([TF])", out)
    assert len(checks) == 14 and all(v == "T" for _, v in checks), out
    n, lowest = 1200, 4
    a = np.diag(1.0 + np.arange(n, dtype=np.float64))
    b = np.eye(n)
    for off, w in ((1, 0.3), (2, 0.15)):
        a += w * (np.eye(n, k=off) + np.eye(n, k=-off))
    for off, w in ((1, 0.05), (2, 0.025)):
        b += w * (np.eye(n, k=off) + np.eye(n, k=-off))
    iters = [int(x) for x in re.search(r"ITERS\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", out).groups()]
    for label, method, bb, it in (("EVALS_DPR", "DPR", None, iters[0]), ("EVALS_GJD", "GJD", None, iters[1]), ("EVALS_GEN", "DPR", b, iters[2])):
        lam_o, _, it_o = O.generalized_eigensolver_dense(a, lowest, method, 1000, 1e-8, 10 * lowest, bb)
        ev = np.array([float(x) for x in re.search(label + r"(.*)", out).group(1).split()])
        assert np.abs(ev - lam_o).max() < 1e-9, label
        assert it == it_o, label
