"""Shared by the tests of the built preconditioner (davp_build_fsai, include/davidson_hip_precond.h; not collected): the banded test
matrix, the canonical store of a CSR input as the engine keeps it, and a numpy restatement of the build - pattern(a, level) and
fsai_rows(a, b, sigma, level), row by row: the gather summing duplicates from +0.0 in stored order, the Cholesky factorisation column by
column (right-looking), z = e_m / l_mm, the back substitution from the last row up and G(i, J) = y / sqrt(y_m), the kernel's operation
order (the kernel contracts a - b * c into one fused operation, numpy rounds twice: the two agree to rounding, not bit for bit).
reference_rows solves every row with numpy.linalg.solve and returns the condition numbers the bound of the tests is made of."""
import numpy as np

import precond_inputs as P

MAX_ROW = 64          # FSAI_MAX_ROW of csrc/kernels.h
EPS = np.finfo(np.float64).eps


# ---- matrices -----------------------------------------------------------------------------------------------------------------------
def banded(n, half_bandwidth=63, seed=5):
    """dense symmetric banded matrix: off-diagonals uniform in (-1, 1) inside the band, diagonal = row sum of |a_ij| + 1 + rand"""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, n))
    for off in range(1, min(half_bandwidth, n - 1) + 1):
        w = 2.0 * rng.random(n - off) - 1.0
        a += np.diag(w, off) + np.diag(w, -off)
    a[np.arange(n), np.arange(n)] = np.abs(a).sum(axis=1) + 1.0 + rng.random(n)
    return a


def banded_csr(n, half_bandwidth=63, seed=5):
    """the banded matrix as full CSR, built without the dense matrix (n = 4097 would take 134 MB): the entries of banded()"""
    rng = np.random.default_rng(seed)
    hb = min(half_bandwidth, n - 1)
    offs = [2.0 * rng.random(n - off) - 1.0 for off in range(1, hb + 1)]
    extra = rng.random(n)
    rows, cols, vals = [], [], []
    for k, w in enumerate(offs, start=1):
        i = np.arange(n - k)
        rows += [i, i + k]
        cols += [i + k, i]
        vals += [w, w]
    absum = np.zeros(n)
    for r, v in zip(rows, vals):
        np.add.at(absum, r, np.abs(v))
    rows.append(np.arange(n)); cols.append(np.arange(n)); vals.append(absum + 1.0 + extra)
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return indptr, cols.astype(np.int32), np.ascontiguousarray(vals)


def lower_with_duplicates(indptr, indices, data, seed=7, every=5):
    """the lower triangle of a full CSR matrix (DAV_CSR_LOWER input), every `every`-th entry split into two terms v = t + (v - t) that
    follow each other: duplicates, separate terms in stored order"""
    rng = np.random.default_rng(seed)
    n = indptr.size - 1
    rp, ci, vv = [0], [], []
    count = 0
    for i in range(n):
        for p in range(indptr[i], indptr[i + 1]):
            if indices[p] > i:
                continue
            count += 1
            if count % every == 0:
                t = float(data[p]) * rng.random()
                ci += [indices[p], indices[p]]
                vv += [t, float(data[p]) - t]
            else:
                ci.append(indices[p])
                vv.append(float(data[p]))
        rp.append(len(ci))
    return np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.array(vv, dtype=np.float64)


def canonical(indptr, indices, data, lower=False):
    """the canonical store the engine keeps of a CSR input (one rank): every row its own entries in input order, then (lower) the
    mirrored strict lower entries in the order of their source rows, stably sorted by column - duplicates stay separate terms"""
    n = indptr.size - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    cols = np.asarray(indices, dtype=np.int64)
    vals = np.asarray(data, dtype=np.float64)
    if lower:
        strict = cols < rows
        rows, cols, vals = (np.concatenate([rows, cols[strict]]), np.concatenate([cols, rows[strict]]),
                            np.concatenate([vals, vals[strict]]))
    order = np.lexsort((np.arange(rows.size), cols, rows))          # by row, then column, then position: a stable sort
    rows, cols, vals = rows[order], cols[order], vals[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return rp, cols.astype(np.int32), np.ascontiguousarray(vals)


def dense_csr(a):
    """canonical store of the non-zeros of a dense symmetric matrix"""
    return canonical(*P.csr_of(a))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def pattern(a, level):
    """(indptr, indices) of P_level: row i = the sorted columns of row i of tril(A)^level (the power of the lower triangle of A), i last"""
    rp, ci, _ = a
    n = rp.size - 1
    p1 = []
    for i in range(n):
        c = ci[rp[i]:rp[i + 1]]
        p1.append(np.union1d(c[c <= i], [i]).astype(np.int64))
    cur = p1
    for _ in range(1, level):
        cur = [np.unique(np.concatenate([p1[j] for j in row])) for row in cur]
    indptr = np.concatenate([[0], np.cumsum([r.size for r in cur])]).astype(np.int64)
    return indptr, np.concatenate(cur).astype(np.int32) if n else np.zeros(0, dtype=np.int32)


def longest_row(pat):
    return int(np.diff(pat[0]).max()) if pat[0].size > 1 else 0


def summed(store):
    """(keys, sums) of a canonical store: keys = row * n + column of the distinct entries, ascending; sums = per distinct entry the sum
    from +0.0 in stored order of its duplicates"""
    rp, ci, vv = store
    n = rp.size - 1
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)) * n + ci
    first = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]])) if keys.size else np.zeros(0, dtype=np.int64)
    sums = np.zeros(first.size)
    ends = np.concatenate([first[1:], [keys.size]])
    width = int((ends - first).max()) if first.size else 0
    for t in range(width):          # term t of every entry that has one: the stored order
        has = first + t < ends
        sums[has] = sums[has] + vv[first[has] + t]
    return n, keys[first], sums


_SUMMED = {}


def _summed_of(store):
    key = id(store[2])
    if key not in _SUMMED or _SUMMED[key][0] is not store[2]:
        _SUMMED[key] = (store[2], summed(store))
    return _SUMMED[key][1]


def _entries(store, cols):
    """the m x m matrix S(J_p, J_q), J = cols, 0.0 where nothing is stored"""
    n, keys, sums = _summed_of(store)
    want = (cols.astype(np.int64)[:, None] * n + cols.astype(np.int64)[None, :]).ravel()
    pos = np.minimum(np.searchsorted(keys, want), max(keys.size - 1, 0))
    hit = keys[pos] == want if keys.size else np.zeros(want.size, dtype=bool)
    return np.where(hit, sums[pos] if keys.size else 0.0, 0.0).reshape(cols.size, cols.size)


def gathered(a, b, sigma, cols):
    """C_JJ = A_JJ - sigma B_JJ from the lower triangles (the upper triangle mirrors them), J = cols; b None: the identity"""
    c = _entries(a, cols) - sigma * (np.eye(cols.size) if b is None else _entries(b, cols))
    low = np.tril(c)
    return low + np.tril(low, -1).T


def row_of_g(c):
    """the row of G from the gathered C_JJ in the kernel's order, or None where a pivot is not finite or not > 0"""
    m = c.shape[0]
    low = np.tril(c).copy()
    for k in range(m):
        d = low[k, k]
        if not (d > 0.0) or not np.isfinite(d):
            return None
        piv = np.sqrt(d)
        low[k + 1:, k] = low[k + 1:, k] / piv
        low[k, k] = piv
        col = low[k + 1:, k]
        low[k + 1:, k + 1:] -= np.tril(np.outer(col, col))
    acc = np.zeros(m)
    acc[m - 1] = 1.0 / low[m - 1, m - 1]
    y = np.zeros(m)
    for q in range(m - 1, -1, -1):
        y[q] = acc[q] / low[q, q]
        acc[:q] -= low[q, :q] * y[q]
    return y / np.sqrt(y[m - 1])


def fsai_rows(a, b, sigma, level, pat=None):
    """(indptr, indices, values, first_bad): the rows of G on pattern(a, level); first_bad = the smallest row with a failed pivot
    (its values and those of every other failed row are NaN) or None"""
    rp, ci = pattern(a, level) if pat is None else pat
    vals = np.full(ci.size, np.nan)
    first_bad = None
    for i in range(rp.size - 1):
        g = row_of_g(gathered(a, b, sigma, ci[rp[i]:rp[i + 1]]))
        if g is None:
            first_bad = i if first_bad is None else first_bad
        else:
            vals[rp[i]:rp[i + 1]] = g
    return rp, ci, vals, first_bad


def reference_rows(a, b, sigma, pat):
    """per row: numpy.linalg.solve of C_JJ y = e_m scaled to G(i, J) = y / sqrt(y_m), and cond_2(C_JJ).  Returns (values, conds)."""
    rp, ci = pat
    vals = np.zeros(ci.size)
    conds = np.zeros(rp.size - 1)
    for i in range(rp.size - 1):
        c = gathered(a, b, sigma, ci[rp[i]:rp[i + 1]])
        e = np.zeros(c.shape[0])
        e[-1] = 1.0
        y = np.linalg.solve(c, e)
        vals[rp[i]:rp[i + 1]] = y / np.sqrt(y[-1])
        conds[i] = np.linalg.cond(c, 2)
    return vals, conds


def row_bounds(pat, ref_vals, conds):
    """per row 8 m^2 eps cond_2(C_JJ) ||g_ref||_2: the normwise bound of a Cholesky solve (Higham, Accuracy and Stability of Numerical
    Algorithms, Theorem 10.4), doubled because the reference carries the same error"""
    rp = pat[0]
    m = np.diff(rp).astype(np.float64)
    norms = np.sqrt(np.add.reduceat(ref_vals * ref_vals, rp[:-1])) if ref_vals.size else np.zeros(0)
    return 8.0 * m * m * EPS * conds * norms


def row_errors(pat, got, ref_vals):
    """per row ||g - g_ref||_2"""
    d = got - ref_vals
    return np.sqrt(np.add.reduceat(d * d, pat[0][:-1])) if d.size else np.zeros(0)


def dense_factor(n, rp, ci, vals):
    g = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(rp))
    g[rows, ci] = vals
    return g


def transpose_csr(n, rp, ci, vals):
    """the CSR arrays of G^T, rows ascending in the column (G holds no duplicates: the order is unique)"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    order = np.lexsort((rows, ci))
    trp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))]).astype(np.int64)
    return trp, rows[order].astype(np.int32), np.ascontiguousarray(vals[order])


# ---- the inputs of the GPU tests, built once ---------------------------------------------------------------------------------------------
T1_SIZES = (1, 17, 300, 4097)
_CACHE = {}


def t1_case(n):
    """(full CSR input, lower input with duplicates) of the banded matrix of order n"""
    if ("t1", n) not in _CACHE:
        full = banded_csr(n)
        _CACHE["t1", n] = (full, lower_with_duplicates(*full))
    return _CACHE["t1", n]


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def level_case(shape, gev):
    """(A dense, B dense | None) of the levels test: the 5-point Laplacian plus potential on a shape[0] x shape[1] grid"""
    def make():
        a = P.hamiltonian(shape[0], shape[1], 0.5, 3)[0]
        return a, P.mass_matrix(a.shape[0], 103) if gev else None
    return cached(("levels", shape, gev), make)


def restated_m(name, level, sigma=0.0):
    """M = G^T G (dense) of a solve case of precond_inputs from the restatement"""
    def make():
        a, b, _, _ = P.solve_case(name)
        rp, ci, vals, bad = fsai_rows(dense_csr(a), None if b is None else dense_csr(b), sigma, level)
        assert bad is None
        g = dense_factor(a.shape[0], rp, ci, vals)
        return g.T @ g
    return cached(("M", name, level, sigma), make)


def restated_iterations(name, level=None):
    """iterations of the restated solve of a case: plain DPR (level None) or with the restated M"""
    def make():
        a, b, _, lowest = P.solve_case(name)
        return P.restated_solve(a, lowest, b, None if level is None else restated_m(name, level))
    return cached(("solve", name, level), make)
