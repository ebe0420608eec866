"""Inputs whose block products are exact, their references, and the write fences around one apply - shared by
tests/test_exact_products_gpu.py.

Exact-integer design: symmetric integer A with |a| <= 255 (exact in fp32 too), integer X with |x| < 2^28, most entries odd and above
2^24 (not representable in fp32), n < 2^17.  Every partial sum of A X in any order is an integer below 2^53, so every schedule, rank
count and inner precision must return the integer product bit for bit: a demoted operand or accumulator, a lost, doubled or misplaced
term changes at least one bit.  Small-magnitude blocks (|x| <= 1) keep W^T W exact as well, which is how the padding rows of a result
are checked through the engine's own Gram product (it sums over the padded rows).

Nothing here asserts while several ranks may still be inside a collective: the fence checks return messages, the callers assert."""
import ctypes as C
import threading
import time

import numpy as np

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import PANEL_R, PANEL_V, PANEL_W, PANEL_X

U64 = 2.0 ** -53
SENTINEL = -0.7265625 * 2.0 ** 70          # exact, never a product of the inputs below
AMAX = 255


def gamma(n, u=U64):
    """gamma_n = n u / (1 - n u): |fl(sum) - sum| <= gamma_n sum |terms| for any order of summation, with or without FMA"""
    return n * u / (1.0 - n * u)


def sym_int_matrix(n, rng, amax=AMAX):
    a = rng.integers(-amax, amax + 1, (n, n))
    a = np.tril(a) + np.tril(a, -1).T
    return np.asfortranarray(a.astype(np.float64))


def int_block(n, k, rng, bits=28):
    """|x| < 2^bits, about 95 % odd and (bits = 28) above 2^24 in magnitude, the rest small (zeros included)"""
    mag = 2 * rng.integers(2 ** (bits - 4), 2 ** (bits - 1) - 1, (n, k)) + 1
    x = np.where(rng.random((n, k)) < 0.5, -mag, mag)
    small = rng.random((n, k)) < 0.05
    x[small] = rng.integers(-3, 4, int(small.sum()))
    return np.asfortranarray(x.astype(np.float64))


def unit_block(n, k, rng):
    return np.asfortranarray(rng.integers(-1, 2, (n, k)).astype(np.float64))


def exact_dense_product(a, x):
    """A X exactly for integer A (|a| <= 255) and X (|x| < 2^28), n < 2^17: X split into 14-bit halves, each BLAS product exact"""
    xi = x.astype(np.int64)
    hi = np.floor_divide(xi, 2 ** 14)
    lo = xi - hi * 2 ** 14
    return np.asfortranarray((a @ hi.astype(np.float64)) * 2.0 ** 14 + a @ lo.astype(np.float64))


def exact_sparse_product(n, rows, cols, vals, x):
    """sum over the stored entries (rows, cols, vals) of vals * X[cols] in int64 (NaN rows of X read as 0)"""
    xi = np.where(np.isnan(x), 0.0, x).astype(np.int64)
    y = np.zeros((n, x.shape[1]), dtype=np.int64)
    np.add.at(y, rows, vals.astype(np.int64)[:, None] * xi[cols])
    return y.astype(np.float64)


def touched_rows(n, rows, cols, nan_rows):
    """output rows whose stored pattern (explicit zeros and duplicates counted) reads a NaN row of X"""
    bad = np.zeros(n, dtype=bool)
    bad[nan_rows] = True
    hit = np.zeros(n, dtype=bool)
    np.logical_or.at(hit, rows, bad[cols])
    return hit


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def mismatch(w, ref):
    """a short description of where two results differ (NaN positions count)"""
    bad = ~((w == ref) | (np.isnan(w) & np.isnan(ref)))
    if not bad.any():
        return "equal"
    i, j = np.argwhere(bad)[0]
    rel = np.abs(w[bad] - ref[bad]) / np.maximum(np.abs(ref[bad]), 1.0)
    return f"{int(bad.sum())} entries differ, first ({i}, {j}): {w[i, j]!r} vs {ref[i, j]!r}, max relative {np.nanmax(rel):.3g}"


def fenced_apply(e, x, c0, d0, cols, apply, stale=0):
    """W = Op X through `apply(src_panel, c0, k, dst_panel, d0)` inside write fences: the source panel NaN in every column but
    [c0, c0 + k), the destination panel SENTINEL in every column; stale > 0 first runs a `stale`-column apply of a NaN block (the packed
    operand then holds NaN groups past the columns of the apply under test).  Returns (W[:, d0:d0 + k], messages): the messages say
    where the source panel changed or destination columns outside [d0, d0 + k) lost the sentinel.  `cols` = columns of a panel."""
    n, k = x.shape
    if stale:
        e.panel_put(PANEL_X, 0, np.full((n, stale), np.nan))
        apply(PANEL_X, 0, stale, PANEL_R, 0)
    src = np.full((n, cols), np.nan, order="F")
    src[:, c0:c0 + k] = x
    e.panel_put(PANEL_V, 0, src)
    e.panel_put(PANEL_W, 0, np.full((n, cols), SENTINEL, order="F"))
    apply(PANEL_V, c0, k, PANEL_W, d0)
    w = e.panel_get(PANEL_W, 0, cols)
    back = e.panel_get(PANEL_V, 0, cols)
    msgs = []
    if not same_bits(back, src):
        msgs.append("the apply wrote into its source panel")
    outside = np.ones(cols, dtype=bool)
    outside[d0:d0 + k] = False
    hit = np.flatnonzero((w[:, outside] != SENTINEL).any(axis=0))
    if hit.size:
        msgs.append(f"destination columns {np.flatnonzero(outside)[hit].tolist()} outside [{d0}, {d0 + k}) were written")
    return np.asfortranarray(w[:, d0:d0 + k]), msgs


def gram_is_exact(g, w):
    """g (the engine's gram of the result columns, summed over the padded rows) equals W^T W exactly - so the padding rows of the
    result are zero.  Needs sum_i w_ij^2 < 2^53 (asserted): then every order of summation is exact."""
    assert (np.sum(w * w, axis=0) < 2.0 ** 53).all()
    return np.array_equal(g, w.T @ w)


def run_ranks(nranks, make, work, timeout=300):
    """nranks engines as threads of this process on one GPU, collectives through the loopback transport (as tests/test_bsr_gpu.py):
    every rank hands its turn on (dav_local_group_yield) when its work ends, whether it raised or not.  A rank that raised before a
    collective leaves its peers in the loopback barrier: their threads are daemons, their engines are NOT closed under them (that
    memory is leaked), and the test fails at once."""
    engs = [make(r) for r in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def run(r):
        try:
            out[r] = work(r, engs[r])
        except Exception as exc:      # noqa: BLE001
            err[r] = exc
        finally:
            fd.hip_lib().dav_local_group_yield(engs[r].h)
    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(nranks)]
    [t.start() for t in threads]
    deadline = time.monotonic() + timeout
    first_error = None
    while any(t.is_alive() for t in threads) and time.monotonic() < deadline:
        if first_error is None and any(x is not None for x in err):
            first_error = time.monotonic()
        if first_error is not None and time.monotonic() > first_error + 10.0:
            break                     # a rank failed 10 s ago and its peers still wait for it
        time.sleep(0.05)
    alive = [r for r, t in enumerate(threads) if t.is_alive()]
    assert not alive, f"ranks {alive} did not finish (errors of the others: {err})"
    for e in engs:
        e.close()
    assert all(x is None for x in err), err
    return out
