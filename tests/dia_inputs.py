"""Shared by the tests of the storage by diagonals (DAV_CSR_DIAGONALS; not collected): the test matrices as symmetric COO triples with
exact-integer values, their CSR input forms, and a numpy restatement of what the engine builds - the canonical order of a CSR set call,
the set of offsets column - row, the slots with duplicates summed in canonical order from +0.0, and the eligibility rule."""
import numpy as np

DIA_MAX_FILL = 4
CSR_FULL, CSR_LOWER, CSR_DIAGONALS = 0, 1, 2


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def flag_word(lower, diagonals):
    return (CSR_LOWER if lower else CSR_FULL) | (CSR_DIAGONALS if diagonals else 0)


def canonical(n, indptr, indices, data, lower=False, base=0):
    """(rows, cols, vals) of the canonical matrix, 0-based, in canonical order: per row the own entries in input order, then (lower) the
    mirrored strict lower entries in the order of their source rows, sorted by column, stable"""
    indptr = np.asarray(indptr, dtype=np.int64) - base
    cols = np.asarray(indices, dtype=np.int64) - base
    vals = np.asarray(data, dtype=np.float64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    pos = np.arange(rows.size, dtype=np.int64)
    if lower:
        below = cols < rows
        rows, cols, vals, pos = (np.concatenate([rows, cols[below]]), np.concatenate([cols, rows[below]]),
                                 np.concatenate([vals, vals[below]]), np.concatenate([pos, pos[below]]))
    order = np.lexsort((pos, cols, rows))          # equal columns of a row: own and mirrored never meet, so input order decides
    return rows[order], cols[order], vals[order]


def offsets(rows, cols):
    """the sorted distinct offsets column - row"""
    return np.unique(cols - rows).astype(np.int32)


def slots(n, rows, cols, vals, offs):
    """val[d][row]: +0.0, or the entries at (row, row + offs[d]) added one after the other in canonical order from +0.0"""
    out = np.zeros((offs.size, n))
    np.add.at(out, (np.searchsorted(offs, cols - rows), rows), vals)       # unbuffered: in the order given
    return out


def eligible(nd, n, entries):
    return nd * n <= DIA_MAX_FILL * max(entries, n)


def dia_product(n, offs, val, x):
    """the product as the kernel orders it: per (row, column) the diagonals in ascending offset from +0.0 (numpy multiplies and adds
    separately, the kernel fuses: equal for exact inputs, within gamma otherwise); a column outside [0, n) reads the clamped row"""
    y = np.zeros((n, x.shape[1]))
    i = np.arange(n)
    for d, off in enumerate(offs):
        y += val[d][:, None] * x[np.clip(i + int(off), 0, n - 1)]
    return y


# ---- matrices -------------------------------------------------------------------------------------------------------------------------
def diagonals_coo(n, offs, rng, amax=255, keep=None):
    """symmetric integer entries |a| <= amax (none zero) on the offsets `offs` >= 0 and their mirror images; keep(d, i): entry (i, i + d)
    is stored"""
    r, c, v = [], [], []
    for d in offs:
        i = np.arange(n - d)
        if keep is not None:
            i = i[keep(d, i)]
        w = rng.integers(1, amax + 1, i.size) * rng.choice([-1, 1], i.size)
        r += [i] if d == 0 else [i, i + d]
        c += [i + d] if d == 0 else [i + d, i]
        v += [w] if d == 0 else [w, w]
    return np.concatenate(r), np.concatenate(c), np.concatenate(v).astype(np.float64)


def stencil7(nx):
    """keep(d, i) of the 7-point stencil of an nx^3 grid: offsets 1, nx, nx^2 with the gaps at the faces"""
    def keep(d, i):
        if d == 0:
            return np.ones(i.size, dtype=bool)
        if d == 1:
            return i % nx != nx - 1
        if d == nx:
            return (i // nx) % nx != nx - 1
        return np.ones(i.size, dtype=bool)
    return keep


def pattern(name):
    """(n, rows, cols, vals) of the T1 patterns: every stored entry of the symmetric matrix, duplicates listed twice"""
    rng = np.random.default_rng(sum(name.encode()))
    if name == "diagonal":
        return (50, *diagonals_coo(50, [0], rng, keep=lambda d, i: i % 7 != 3))
    if name == "tridiagonal":
        return (50, *diagonals_coo(50, [0, 1], rng))
    if name == "stencil":
        return (343, *diagonals_coo(343, [0, 1, 7, 49], rng, keep=stencil7(7)))
    if name == "band65":
        return (301, *diagonals_coo(301, list(range(33)), rng))
    if name == "corners":
        return (777, *diagonals_coo(777, [0, 1, 776], rng))
    if name == "empty_row_duplicates":
        n = 301
        r, c, v = diagonals_coo(n, [0, 1], rng)
        gone = (r == 100) | (c == 100)                               # row (and column) 100 is empty
        r, c, v = r[~gone], c[~gone], v[~gone]
        i = np.array([0, 17, 18, 200, 299])                          # duplicates of (i, i + 1) / (i + 1, i) and of two diagonal entries
        w = rng.integers(1, 256, i.size).astype(np.float64)
        dd = np.array([5, 300])
        wd = rng.integers(1, 256, dd.size).astype(np.float64)
        return n, np.concatenate([r, i, i + 1, dd]), np.concatenate([c, i + 1, i, dd]), np.concatenate([v, w, w, wd])
    raise KeyError(name)


PATTERNS = ("diagonal", "tridiagonal", "stencil", "band65", "corners", "empty_row_duplicates")


def csr_form(n, rows, cols, vals, lower=False, base=0):
    """(indptr int64, indices int32, data) of the COO triples, stable by row (duplicates and their order kept); lower: column <= row"""
    if lower:
        keep = cols <= rows
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.argsort(rows, kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order]
    indptr = np.searchsorted(rows, np.arange(n + 1)).astype(np.int64)
    return indptr + base, (cols + base).astype(np.int32), vals.astype(np.float64)


def csr_of_dense(a, lower=False):
    """(indptr, indices, data) of the non-zeros of a dense symmetric matrix"""
    rows, cols = np.nonzero(a)
    return csr_form(a.shape[0], rows, cols, a[rows, cols], lower)
