"""Inputs of the Hermitian tests (test_herm_cpu.py, test_herm_gpu.py, test_herm_fortran.py): complex Hermitian CSR matrices of the six
pattern classes of test_sparse_gpu.py, their expanded 2 x 2 blocks and real forms as numpy states them, the matrices of the solves, the
bounds the extraction is held to - and the matrices tests/fortran/prog_herm.f90 builds, rebuilt here from the same integer formulas."""
import numpy as np

from test_sparse_gpu import coo_to_csr, symmetric_coo

CLASSES = ("banded", "random", "empty_rows", "missing_diagonal", "duplicates", "arrowhead")


def phase_part(rows, cols, scale):
    """the imaginary part of entry (i, j) next to a real part of magnitude `scale`: a fixed function of the unordered pair, odd under
    the exchange of i and j and +0.0 on the diagonal - so the terms of (j, i) are the conjugates of the terms of (i, j), duplicates too"""
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    g = ((lo * 7919 + hi * 104729) % 2003) / 1001.0 - 1.0          # in [-1, 1]
    im = scale * g * np.sign(rows - cols)
    return np.where(rows == cols, 0.0, im)


def hermitian_csr(n, kind, lower, seed=None, integer=False):
    """(indptr int64, indices int64, data complex128) of a Hermitian matrix of order n of the class `kind`, every nonzero or (lower)
    only the entries with column <= row, the entries of a row shuffled.  integer: real and imaginary parts integers with |.| <= 255."""
    rng = np.random.default_rng(CLASSES.index(kind) * 10 + lower if seed is None else seed)
    if n == 1:          # the classes at order 1: no entry at all, one diagonal entry, or two terms of it
        k = {"empty_rows": 0, "missing_diagonal": 0, "duplicates": 2}.get(kind, 1)
        rows, cols, vals = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64), np.array([0.75, 0.25][:k]) if k == 2 else np.ones(k)
    else:
        rows, cols, vals = (np.asarray(a) for a in symmetric_coo(n, kind, rng))
    rows, cols = rows.astype(np.int64), cols.astype(np.int64)
    if integer:
        lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
        re = ((lo * 31 + hi * 17) % 511 - 255).astype(np.float64)
        im = np.where(rows == cols, 0.0, ((lo * 13 + hi * 29) % 511 - 255) * np.sign(rows - cols)).astype(np.float64)
    else:
        re, im = vals, phase_part(rows, cols, np.abs(vals))
    data = re + 1j * im
    if lower:
        sel = cols <= rows
        rows, cols, data = rows[sel], cols[sel], data[sel]
    p = rng.permutation(rows.size)
    rows, cols, data = rows[p], cols[p], data[p]
    order = np.argsort(rows, kind="stable")
    indptr = np.searchsorted(rows[order], np.arange(n + 1)).astype(np.int64)
    return indptr, cols[order], np.ascontiguousarray(data[order])


def expand_blocks(data):
    """blocks[p] = [[a, -b], [b, a]] of data[p] = a + ib: (nnz, 2, 2), row-major"""
    a, b = data.real, data.imag
    return np.ascontiguousarray(np.stack([np.stack([a, -b], axis=1), np.stack([b, a], axis=1)], axis=1))


def csr_dense(n, indptr, indices, data, lower=False):
    """the dense Hermitian matrix of the arrays (duplicates summed; lower: the strict lower part mirrored as conjugates)"""
    rows = np.repeat(np.arange(n), np.diff(indptr))
    h = np.zeros((n, n), dtype=np.complex128)
    np.add.at(h, (rows, indices), data)
    if lower:
        off = rows != indices
        np.add.at(h, (indices[off], rows[off]), np.conj(data[off]))
    return h


def dense_csr(h, lower=False):
    """(indptr, indices, data) of the nonzeros of a dense Hermitian matrix (lower: column <= row only)"""
    m = np.tril(h) if lower else h
    rows, cols = np.nonzero(m)
    return coo_to_csr_complex(h.shape[0], rows, cols, m[rows, cols])


def coo_to_csr_complex(n, rows, cols, vals):
    order = np.argsort(rows, kind="stable")
    indptr = np.searchsorted(rows[order], np.arange(n + 1)).astype(np.int64)
    return indptr, cols[order].astype(np.int64), np.ascontiguousarray(vals[order], dtype=np.complex128)


def real_form(h):
    """the real symmetric form of order 2 n: v[2 i] = Re x_i, v[2 i + 1] = Im x_i"""
    n = h.shape[0]
    a = np.zeros((2 * n, 2 * n))
    a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2] = h.real, -h.imag, h.imag, h.real
    return a


def interleave(x):
    """the real form of complex columns"""
    v = np.zeros((2 * x.shape[0],) + x.shape[1:])
    v[0::2], v[1::2] = x.real, x.imag
    return v


# ---- the extraction ------------------------------------------------------------------------------------------------------------------
def extraction_case(case, n=40, lowest=4, seed=0):
    """(H, S | None) of the three cases: generic; pencil (S = I + a small Hermitian part); cluster_cut (a triple eigenvalue across the
    cut: positions lowest - 1, lowest, lowest + 1)"""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    h = (m + m.conj().T) / 2
    s = None
    if case == "cluster_cut":
        w, q = np.linalg.eigh(h)
        w[lowest - 1] = w[lowest] = w[lowest + 1]
        h = (q * w) @ q.conj().T
        h = (h + h.conj().T) / 2
    if case == "pencil":
        m = 0.02 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
        s = np.eye(n) + (m + m.conj().T) / 2
    return h, s


def extraction_bound(a, b, v, theta):
    """||A V - B V Theta||_F + the largest split of a pair theta[2k], theta[2k + 1]: what the complex residual is held to (times 2)"""
    bv = v if b is None else b @ v
    return np.linalg.norm(a @ v - bv * theta[None, :]) + np.abs(theta[0::2] - theta[1::2]).max()


def check_extraction(h, s, theta, v, lam, x, ref, tol_lambda=1e-12, show=print):
    """the three assertions of the extraction on (lam, x) taken from the real-form pairs (theta, v); ref: eigh's eigenvalues"""
    lowest = lam.size
    sx = x if s is None else s @ x
    dlam = np.abs(lam - ref[:lowest]).max()
    orth = np.abs(x.conj().T @ sx - np.eye(lowest)).max()
    res = np.linalg.norm(h @ x - sx * lam[None, :], axis=0).max()
    bound = 2.0 * extraction_bound(real_form(h), None if s is None else real_form(s), v, theta)
    show(f"extraction: |lambda - eigh| {dlam:.3g}, |X^H S X - I| {orth:.3g}, residual {res:.3g} against the bound {bound:.3g}")
    if tol_lambda is not None:
        assert dlam <= tol_lambda, dlam
    assert orth <= 1e-12, orth
    assert res <= bound, (res, bound)


# ---- the matrices of the solves (n_c = 200 - the lattice 400 -, lowest 4) ----------------------------------------------------------------------------------
def solve_matrix(name, n=200, seed=3):
    """(H, S | None) dense: graded - a random Hermitian matrix with a graded diagonal; pencil - the same with S = I + a small Hermitian
    part; double - a spectrum with an exact double eigenvalue at the cut (pairs 4 and 5 of 1-based order); lattice - a 20 x 20 square
    lattice with Peierls phases (flux 1 / 8 per plaquette, Landau gauge) in a harmonic trap, with a weak on-site term that lifts the symmetries"""
    rng = np.random.default_rng(seed)
    if name == "lattice":
        nx = 20
        n = nx * nx          # the lattice has its own order: 400 sites
        h = np.zeros((n, n), dtype=np.complex128)
        idx = lambda ix, iy: ix * nx + iy          # noqa: E731
        for ix in range(nx):
            for iy in range(nx):
                h[idx(ix, iy), idx(ix, iy)] = 4.0 + 0.3 * ((37 * idx(ix, iy) + 11) % 101) / 101.0 + 0.02 * ((ix - 9.5) ** 2 + (iy - 9.5) ** 2)
                if iy + 1 < nx:
                    h[idx(ix, iy), idx(ix, iy + 1)] = h[idx(ix, iy + 1), idx(ix, iy)] = -1.0
                if ix + 1 < nx:
                    t = -np.exp(2j * np.pi * 0.125 * iy)
                    h[idx(ix + 1, iy), idx(ix, iy)] = t
                    h[idx(ix, iy), idx(ix + 1, iy)] = np.conj(t)
        return h, None
    mask = rng.random((n, n)) < 0.05
    m = np.where(mask, 0.05 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))), 0.0)
    h = np.tril(m, -1)
    h = h + h.conj().T + np.diag(1.0 + np.arange(n, dtype=np.float64))
    s = None
    if name == "pencil":
        ms = np.where(rng.random((n, n)) < 0.03, 0.01 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))), 0.0)
        s = np.tril(ms, -1)
        s = s + s.conj().T + np.eye(n)
    if name == "double":          # two decoupled copies of one small Hermitian block at the bottom of the spectrum give pairs 4 and 5 one value
        blk = np.array([[4.0, 0.05 + 0.02j], [0.05 - 0.02j, 4.7]])
        h[3:7, :] = 0.0
        h[:, 3:7] = 0.0
        h[3:5, 3:5] = blk
        h[5:7, 5:7] = blk
    return h, s


# ---- tests/fortran/prog_herm.f90 --------------------------------------------------------------------------------------------------------
def fortran_matrix(nx=12):
    """the Peierls lattice the program builds (1-based site p = (ix - 1) nx + iy): on-site 4 + 0.3 mod(37 p + 11, 101) / 101 + 0.05 ((ix - 6.5)^2 + (iy - 6.5)^2), hopping -1
    along y, -exp(2 pi i iy / 8) along x (entry (p + nx, p))"""
    n = nx * nx
    h = np.zeros((n, n), dtype=np.complex128)
    for ix in range(1, nx + 1):
        for iy in range(1, nx + 1):
            p = (ix - 1) * nx + iy
            h[p - 1, p - 1] = 4.0 + 0.3 * ((37 * p + 11) % 101) / 101.0 + 0.05 * ((ix - 6.5) ** 2 + (iy - 6.5) ** 2)
            if iy < nx:
                h[p, p - 1] = h[p - 1, p] = -1.0
            if ix < nx:
                t = -np.exp(2j * np.pi * iy / 8.0)
                h[p + nx - 1, p - 1] = t
                h[p - 1, p + nx - 1] = np.conj(t)
    return h


def fortran_overlap(nx=12):
    """S of the program's pencil: 1 on the diagonal, 0.05 i along y (entry (p + 1, p)) and its conjugate"""
    n = nx * nx
    s = np.eye(n, dtype=np.complex128)
    for ix in range(1, nx + 1):
        for iy in range(1, nx):
            p = (ix - 1) * nx + iy
            s[p, p - 1] = 0.05j
            s[p - 1, p] = -0.05j
    return s
