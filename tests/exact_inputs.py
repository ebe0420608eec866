"""Inputs whose block products are exact, their references, and the write fences around one apply - shared by
tests/test_exact_products_gpu.py; behind them the integer inputs, references and the numpy restatement of the GJD correction that
tests/test_exact_phases_gpu.py holds the other phases of an outer iteration to (tests/test_exact_phase_inputs_cpu.py checks those).

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


# ---- the phases of an outer iteration besides the block products (tests/test_exact_phases_gpu.py) ------------------------------------
# Exact-integer design of parts A - C: every panel holds integers, every small matrix the host builds from the caller's (-Y theta,
# -C M) is an exact integer product, and every partial sum of a panel product stays below 2^53 (test_exact_phase_inputs_cpu.py checks
# the bounds on the generated inputs), so any order of summation, with or without FMA, returns the integer result bit for bit.
#   wide:   panels from int_block(bits=20), |y| <= 7, integer 1 <= |theta| <= 8:  |X| < 128 2^20 7 < 2^30, |R| <= 128 2^20 63 < 2^33
#   narrow: panels from unit_block, |y| <= 3, theta in {+-1, +-2}:  |R| <= 128 (3 + 6) = 1152, R^2 < 2^22, and with n < 2^14 the squared
#           norms are exact integers below 2^36 - the host's one sqrt of them is correctly rounded
def cols_alloc(max_cols):
    """columns of every panel of an engine created with max_cols (dav_create)"""
    return (max_cols + 15) // 16 * 16 + 16


def int_matrix(p, q, rng, amax=7):
    return np.asfortranarray(rng.integers(-amax, amax + 1, (p, q)).astype(np.float64))


def int_product(p, m):
    """P M for integer-valued float64 P and M, in int64"""
    return p.astype(np.int64) @ m.astype(np.int64)


def phase_block(kind, n, k, rng):
    return unit_block(n, k, rng) if kind == "narrow" else int_block(n, k, rng, bits=20)


def ritz_inputs(kind, n, m, ncorr, gev, rng, dyadic=False):
    """(V, W, Z, Y, theta) of one Ritz phase: Z = V, or the B V panel when gev.  dyadic: |theta| a power of two"""
    v, w = phase_block(kind, n, m, rng), phase_block(kind, n, m, rng)
    z = phase_block(kind, n, m, rng) if gev else v
    y = int_matrix(m, ncorr, rng, 3 if kind == "narrow" else 7)
    mags = [1, 2] if kind == "narrow" else [1, 2, 4, 8] if dyadic else list(range(1, 9))
    theta = rng.choice(mags, ncorr) * rng.choice([-1, 1], ncorr)
    return v, w, z, y, theta.astype(np.float64)


def ritz_reference(v, w, z, y, theta):
    """(X = V Y, R = W Y + Z (-Y theta), squared column norms of R) in int64"""
    yi = y.astype(np.int64)
    x = v.astype(np.int64) @ yi
    r = w.astype(np.int64) @ yi + z.astype(np.int64) @ (-(yi * theta.astype(np.int64)[None, :]))
    return x, r, np.sum(r * r, axis=0)


def dpr_diagonals(n, gev, theta, rng, jstar=None):
    """integer diagonals (dA, dB | None).  jstar None: the dyadic set - dA = 0, dB in {1, 2, 4}, every denominator theta_j dB_i a power of
    two.  Otherwise dA in [-40, 40] with theta_jstar dB_i == dA_i in the guard rows (also returned): the first row, the last, and
    the rows on both sides of every 128-row block edge up to three blocks"""
    db = rng.choice([1.0, 2.0, 4.0], n) if gev else None
    if jstar is None:
        return np.zeros(n), db, np.zeros(0, dtype=np.int64)
    da = rng.integers(-40, 41, n).astype(np.float64)
    rows = np.array(sorted({r for r in (0, 127, 128, 255, 256, 383, n // 2, n - 1) if 0 <= r < n}))
    da[rows] = theta[jstar] * (db[rows] if gev else 1.0)
    return da, db, rows


def dpr_reference(r, theta, da, db):
    """T = R / (theta_j dB_i - dA_i), exactly 0 where the denominator is 0: numpy's correctly rounded fp64 division"""
    den = theta[None, :] * (db[:, None] if db is not None else 1.0) - da[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asfortranarray(np.where(den != 0.0, r.astype(np.float64) / den, 0.0)), den


def fenced(n, cols, fill, c0=0, block=None):
    """an n x cols panel of `fill` with `block` in the columns from c0"""
    p = np.full((n, cols), fill, order="F")
    if block is not None:
        p[:, c0:c0 + block.shape[1]] = block
    return p


# ---- the GJD correction at fixed step counts --------------------------------------------------------------------------------------------
def tridiag_csr(d, off):
    """(indptr, indices, data) of the symmetric tridiagonal matrix with diagonal d and off-diagonal off (off[i] couples rows i, i + 1)"""
    n = d.size
    i = np.arange(n)
    rows = np.concatenate([i, i[:-1], i[1:]])
    cols = np.concatenate([i, i[1:], i[:-1]])
    vals = np.concatenate([d, off, off])
    order = np.lexsort((cols, rows))
    indptr = np.searchsorted(rows[order], np.arange(n + 1)).astype(np.int64)
    return indptr, cols[order].astype(np.int32), vals[order].astype(np.float64)


def tridiag_mul(d, off, v):
    y = d[:, None] * v
    y[:-1] += off[:, None] * v[1:]
    y[1:] += off[:, None] * v[:-1]
    return y


class GjdInputs:
    """One block of projected systems for dav_gjd_correction_n, from a seeded default_rng: A tridiagonal with dA_i = 1 + 8 i / n + U(0, 1)
    and off-diagonals 0.25 N(0, 1); generalized: B tridiagonal with dB_i = 1 + 0.1 U(0, 1) and off-diagonals 0.02 N(0, 1); X = qr(N(0, 1))
    used as it is; R = 1e-2 N(0, 1) (zero_cols: exactly zero); theta_j = 0.5 + 0.05 j.  floor: row i0 = n // 2 has dA_i0 = theta_0 dB_i0
    (the preconditioner's 1e-10 floor in column 0), X[i0, :] = 0 and R[i0, 0] = 2^-40."""

    def __init__(self, n, m, gev, seed, zero_cols=(), floor=False):
        rng = np.random.default_rng(seed)
        self.n, self.m, self.gev = n, m, gev
        self.da = 1.0 + 8.0 * np.arange(n) / n + rng.random(n)
        self.offa = 0.25 * rng.standard_normal(n - 1)
        self.db = 1.0 + 0.1 * rng.random(n) if gev else None
        self.offb = 0.02 * rng.standard_normal(n - 1) if gev else None
        self.x = np.asfortranarray(np.linalg.qr(rng.standard_normal((n, m)))[0])
        self.r = np.asfortranarray(1e-2 * rng.standard_normal((n, m)))
        self.r[:, list(zero_cols)] = 0.0
        self.theta = 0.5 + 0.05 * np.arange(m)
        if floor:
            i0 = n // 2
            self.da[i0] = self.theta[0] * (self.db[i0] if gev else 1.0)
            self.x[i0, :] = 0.0
            self.r[i0, 0] = 2.0 ** -40

    def set_operators(self, e):
        from fortran_davidson_amd.engine_c import OP_A, OP_B
        e.set_operator_csr(OP_A, *tridiag_csr(self.da, self.offa))
        if self.gev:
            e.set_operator_csr(OP_B, *tridiag_csr(self.db, self.offb))

    def restate(self, steps, dtype, inner_tol=0.0):
        t = dtype
        mul_a = lambda v: tridiag_mul(self.da.astype(t), self.offa.astype(t), v)          # noqa: E731
        mul_b = (lambda v: tridiag_mul(self.db.astype(t), self.offb.astype(t), v)) if self.gev else None
        return gjd_restatement(mul_a, mul_b, self.da, self.db, self.x, self.r, self.theta, steps, t, inner_tol)


def gjd_restatement(mul_a, mul_b, da, db, x, r, theta, max_inner, dtype=np.float64, inner_tol=0.0):
    """dav_gjd_correction_n (csrc/engine_gjd.hip) restated in numpy at precision `dtype`: block MINRES on
    (I - x x^T)(A - theta B)(I - x x^T) t = -r with the Jacobi preconditioner K = max(|dA - theta dB|, 1e-10) restricted to the
    complement of x.  mul_a / mul_b: v -> A v / B v on an n x m block of `dtype` (mul_b None: B = I).  Returns (T, steps taken)."""
    t = dtype
    x, r1, th = x.astype(t), -r.astype(t), theta.astype(t)
    n, m = x.shape
    one, zero = t(1.0), t(0.0)
    kd = np.maximum(np.abs(da.astype(t)[:, None] - th[None, :] * (db.astype(t)[:, None] if db is not None else one)), t(1e-10))
    dot = lambda a, b: np.sum(a * b, axis=0)                                             # noqa: E731
    r2 = r1.copy()
    mx, y = x / kd, r1 / kd                                   # the Jacobi preconditioner, with its floor
    xmx = dot(x, mx)
    cy = np.where(xmx > 0, -dot(x, y) / np.where(xmx > 0, xmx, one), zero)              # the projection coefficient
    b2 = dot(r1, y) + cy * dot(r1, mx)
    beta1 = np.where(b2 > 0, np.sqrt(np.maximum(b2, zero)), zero)
    beta, phibar = beta1.copy(), beta1.copy()
    active = beta1 > 0                                        # a column with beta1 == 0 never starts
    oldb, dbar, epsln = np.zeros(m, t), np.zeros(m, t), np.zeros(m, t)
    cs, sn = -np.ones(m, t), np.zeros(m, t)
    tt, w, w1, w2 = (np.zeros((n, m), t) for _ in range(4))
    stall = np.zeros(m, dtype=int)
    itn = 0
    while itn < max_inner and active.any():
        itn += 1
        act = active.astype(t)
        safe_beta = np.where(active, beta, one)
        c0 = act / safe_beta
        v = c0 * y + (c0 * cy) * mx
        ua = mul_a(v)
        ub = mul_b(v) if mul_b is not None else v
        # the Lanczos step, the four-term update: y = (A v - theta B v) - (x^T (A v - theta B v)) x - (beta / oldb) r1
        c2 = -(dot(x, ua) - th * dot(x, ub)) * act
        c3 = np.where(active & (itn >= 2), -beta / np.where(oldb != 0, oldb, one), zero)
        y = act * ua + (-th * act) * ub + c2 * x + c3 * r1
        alfa = dot(v, y)
        y = act * y + np.where(active, -alfa / safe_beta, zero) * r2
        r1, r2 = r2, y
        y = act * (r2 / kd)
        xy, ry, rmx = dot(x, y), dot(r2, y), dot(r2, mx)
        # the Paige - Saunders scalars, per column
        cy = np.where(active, -xy / np.where(xmx != 0, xmx, one), cy)
        b2 = ry + cy * rmx
        oldb = np.where(active, beta, oldb)
        beta = np.where(active, np.where(b2 > 0, np.sqrt(np.maximum(b2, zero)), zero), beta)
        oldeps = np.where(active, epsln, zero)
        delta = np.where(active, cs * dbar + sn * alfa, zero)
        gbar = sn * dbar - cs * alfa
        epsln = np.where(active, sn * beta, epsln)
        dbar = np.where(active, -cs * beta, dbar)
        gam = np.where(active, np.maximum(np.sqrt(gbar * gbar + beta * beta), t(1e-300)), one)
        cs = np.where(active, gbar / gam, cs)
        sn = np.where(active, beta / gam, sn)
        phi = np.where(active, cs * phibar, zero)
        stall = np.where(active, np.where(sn > 0.95, stall + 1, 0), stall)
        phibar = np.where(active, sn * phibar, phibar)
        # w_new = (v - oldeps w1 - delta w2) / gamma;  t += phi w_new
        w1, w2 = w2, w
        w = (act / gam) * v + (-oldeps * act / gam) * w1 + (-delta * act / gam) * w2
        tt = tt + (phi * act) * w
        active = active & (phibar > t(inner_tol) * beta1) & (beta > 0) & ~((stall >= 8) & (phibar < t(1e-6) * beta1))
    return tt, itn


def gjd_error(t, t_ref):
    """max over the columns of ||T_j - Tref_j||_inf / ||Tref_j||_inf (a column of the reference that is entirely zero: 0 if T's is
    too, inf otherwise)"""
    worst = 0.0
    for j in range(t_ref.shape[1]):
        scale = np.max(np.abs(t_ref[:, j]))
        err = np.max(np.abs(t[:, j].astype(np.longdouble) - t_ref[:, j]))
        worst = max(worst, float(err / scale) if scale > 0 else (0.0 if err == 0 else np.inf))
    return worst
