"""Shared by the tests of the Chebyshev-filtered correction (method "CHEB"; not collected): the test matrices, a numpy restatement of the
correction in any floating-point type - interval rule, coefficients, recurrence - the filter evaluated directly, and a restatement of the
solve: the oracle's dense loops (oracle/davidson_oracle.py: generalized_eigensolver_dense and its "unconverged" variant) with only the
correction swapped."""
import numpy as np

from oracle import davidson_oracle as O
import bdpr_inputs as BI

U = 2.0 ** -53
DEFAULT_DEGREE = 10


# ---- matrices -----------------------------------------------------------------------------------------------------------------------
def laplacian2d(nx, seed=None, sigma=0.05, grade=0.0):
    """the 5-point Laplacian of an nx x nx grid (Dirichlet), dense; its diagonal 4 + sigma N(0, 1) (seeded) + grade i / n"""
    n = nx * nx
    a = np.zeros((n, n))
    for i in range(nx):
        for j in range(nx):
            p = i * nx + j
            if j + 1 < nx:
                a[p, p + 1] = a[p + 1, p] = -1.0
            if i + 1 < nx:
                a[p, p + nx] = a[p + nx, p] = -1.0
    d = 4.0 + grade * np.arange(n) / n
    if seed is not None:
        d = d + sigma * np.random.default_rng(seed).standard_normal(n)
    a[np.arange(n), np.arange(n)] = d
    return a


def random_sparse(n, density, seed, grade=0.1):
    """a random symmetric sparse matrix with a graded diagonal 1 + grade i"""
    rng = np.random.default_rng(seed)
    m = np.where(rng.random((n, n)) < density, rng.standard_normal((n, n)), 0.0)
    a = np.triu(m, 1)
    a = a + a.T
    a[np.arange(n), np.arange(n)] = 1.0 + grade * np.arange(n)
    return a


# name -> (matrix, lowest): the inputs of the iteration-count table
def table_inputs():
    return {"lap16_l4": (laplacian2d(16, 1), 4), "lap24_l8": (laplacian2d(24, 2), 8), "lap16_l1": (laplacian2d(16, 1), 1),
            "lap30_graded_l4": (laplacian2d(30, None, grade=1e-3), 4), "block240_b4": (BI.block_matrix(240, 4, 1)[0], 4),
            "block256_b16": (BI.block_matrix(256, 16, 3)[0], 4), "random300": (random_sparse(300, 0.05, 7, grade=0.01), 4)}


MAX_ITERATIONS = 400
# CPU restatement, tolerance 1e-8, max_dim 10 * lowest, at most 400 iterations (401 = not converged):
# name -> {policy: (DPR, CHEB6, CHEB10, CHEB16)}
TABLE = {
    "lap16_l4": {"all": (122, 15, 10, 6), "unconverged": (67, 17, 12, 7)},
    "lap24_l8": {"all": (166, 16, 10, 7), "unconverged": (88, 17, 12, 8)},
    "lap16_l1": {"all": (314, 20, 14, 8), "unconverged": (133, 18, 12, 8)},
    "lap30_graded_l4": {"all": (401, 30, 18, 11), "unconverged": (163, 24, 16, 12)},
    "block240_b4": {"all": (56, 16, 10, 6), "unconverged": (50, 19, 12, 7)},
    "block256_b16": {"all": (51, 18, 11, 7), "unconverged": (47, 18, 11, 8)},
    "random300": {"all": (128, 19, 12, 8), "unconverged": (68, 18, 13, 8)},
}


# ---- the correction -----------------------------------------------------------------------------------------------------------------
def csr_of(a, lower=False):
    """(indptr int64, indices int32, data) of the non-zeros of the dense matrix a (lower: those with column <= row)"""
    mask = a != 0.0
    if lower:
        mask &= np.tril(np.ones_like(mask))
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(mask)
    return indptr, cols.astype(np.int32), a[rows, cols].astype(np.float64)


def row_bound(a):
    """the largest row sum of |a_ij| as the engine takes it from the stored operator: a row's stored entries added one after the other
    in column order from +0.0 (zeros add nothing, so this is the dense row's sum in that order; stored duplicates are beyond a dense
    matrix)"""
    best = 0.0
    for row in np.abs(np.asarray(a, dtype=np.float64)):
        nz = row[row != 0.0]
        if nz.size:
            best = max(best, float(np.add.accumulate(nz)[-1]))
    return best


class Product:
    """A z in the floating-point type of z, from the non-zeros of the dense matrix a (numpy has no fast long-double matmul)"""

    def __init__(self, a):
        self.n = a.shape[0]
        rows, cols = np.nonzero(a)
        self.cols, self.vals = cols, a[rows, cols]
        counts = np.bincount(rows, minlength=self.n)
        self.filled = np.flatnonzero(counts)
        self.starts = (np.cumsum(counts) - counts)[self.filled]

    def __call__(self, z):
        out = np.zeros_like(z)
        if self.vals.size:
            out[self.filled] = np.add.reduceat(self.vals.astype(z.dtype)[:, None] * z[self.cols], self.starts, axis=0)
        return out


def interval(theta, ncorr, lowest, bound, dtype=np.float64):
    """(usable, a0, a, b) of the interval rule: a0 = theta_0, delta = (b - a0) / 64,
    a = min(max(theta_{min(ncorr, 2 lowest) - 1}, theta_{lowest - 1} + delta), b - delta); usable when b and theta[:ncorr] are finite
    and a0 < a < b"""
    th = np.asarray(theta[:ncorr], dtype=dtype)
    b, a0 = dtype(bound), th[0]
    with np.errstate(all="ignore"):
        ok = bool(np.isfinite(b) and np.isfinite(th).all() and b > a0)
        delta = (b - a0) / dtype(64)
        a = min(max(th[min(ncorr, 2 * lowest) - 1], th[lowest - 1] + delta), b - delta)
        ok = ok and bool(a > a0 and b > a)
    return ok, a0, a, b


def cheb_correction(a, theta, r, ncorr, lowest, degree, bound=None, dtype=np.float64, product=None):
    """z_d of the recurrence of include/davidson_hip.h for the columns j < ncorr of r, in `dtype`; an unusable interval gives zeros.
    a: dense symmetric matrix; bound: its row-sum bound as the engine forms it (default row_bound(a))"""
    prod = product or (Product(a) if dtype != np.float64 else (lambda z: a @ z))
    ok, a0, lo, b = interval(theta, ncorr, lowest, row_bound(a) if bound is None else bound, dtype)
    rr = np.asarray(r[:, :ncorr], dtype=dtype)
    if not ok:
        return np.zeros_like(rr)
    th = np.asarray(theta[:ncorr], dtype=dtype)
    two = dtype(2)
    c, e = (lo + b) / two, (b - lo) / two
    s1 = e / (a0 - c)
    sk = s1
    pim, pik = np.ones(ncorr, dtype=dtype), (s1 / e) * (th - c)
    zm, zk = np.zeros_like(rr), (s1 / e) * rr
    for _ in range(1, degree):
        sn = dtype(1) / (two / s1 - sk)
        alpha, beta = two * sn / e, sk * sn
        zn = alpha * (prod(zk) - c * zk + pik[None, :] * rr) - beta * zm
        pin = alpha * (th - c) * pik - beta * pim
        zm, zk, pim, pik, sk = zk, zn, pik, pin, sn
    return zk


def filter_direct(a, theta, x, ncorr, lowest, degree, bound=None, dtype=np.longdouble):
    """p_d(A) x_j - p_d(theta_j) x_j with the scaled Chebyshev polynomial of Zhou and Saad for the same interval, evaluated as such:
    y_0 = x, y_1 = (s_1 / e)(A - c) x, y_{k+1} = (2 s_{k+1} / e)(A - c) y_k - s_k s_{k+1} y_{k-1}, and the same recurrence on the number
    theta_j"""
    prod = Product(a)
    ok, a0, lo, b = interval(theta, ncorr, lowest, row_bound(a) if bound is None else bound, dtype)
    assert ok
    xx = np.asarray(x[:, :ncorr], dtype=dtype)
    th = np.asarray(theta[:ncorr], dtype=dtype)
    two = dtype(2)
    c, e = (lo + b) / two, (b - lo) / two
    s1 = e / (a0 - c)
    sk = s1
    ym, yk = xx, (s1 / e) * (prod(xx) - c * xx)
    pm, pk = np.ones(ncorr, dtype=dtype), (s1 / e) * (th - c)
    for _ in range(1, degree):
        sn = dtype(1) / (two / s1 - sk)
        yn = (two * sn / e) * (prod(yk) - c * yk) - sk * sn * ym
        pn = (two * sn / e) * (th - c) * pk - sk * sn * pm
        ym, yk, pm, pk, sk = yk, yn, pk, pn, sn
    return yk - pk[None, :] * xx


# ---- the solve ----------------------------------------------------------------------------------------------------------------------
def method_degree(method):
    """None for "DPR", the degree of "CHEB" / "CHEB<d>" """
    if method == "DPR":
        return None
    assert method.startswith("CHEB")
    return int(method[4:]) if method[4:] else DEFAULT_DEGREE


def restated_solve(a, lowest, method, policy="all", max_iterations=MAX_ITERATIONS, tolerance=1e-8):
    """generalized_eigensolver_dense (policy "all") or generalized_eigensolver_dense_unconverged (policy "unconverged") of the oracle for
    a standard problem, statement by statement, with the correction `method`: "DPR" (scalar, guarded as the engine guards it) or "CHEB" /
    "CHEB<d>".  As in the engine the Chebyshev block of the "unconverged" policy is made for all `lowest` wanted pairs (ncorr = lowest)
    and the columns of the pairs still above the tolerance are taken from it.  Returns (eigenvalues, eigenvectors, iters)."""
    n = a.shape[0]
    degree = method_degree(method)
    bound = row_bound(a)
    initial_dimension, max_dim = 2 * lowest, 10 * lowest
    has_converged = np.zeros(lowest, dtype=bool)
    V = O.generate_preconditioner(O.diagonal(a), initial_dimension)
    H = V.T @ (a @ V)
    eigenvalues, eigenvectors, iters = np.zeros(lowest), np.zeros((n, lowest), order="F"), max_iterations + 1
    for i in range(1, max_iterations + 1):
        theta, Y = O.lapack_generalized_eigensolver(H, None)
        m = V.shape[1]
        ncorr = m if policy == "all" else lowest
        if policy == "all":
            X = V @ Y
            R = np.empty((n, m), order="F")
            for j in range(m):
                R[:, j] = a @ X[:, j] - theta[j] * X[:, j]
        else:
            X = np.asfortranarray(V @ Y[:, :lowest])
            R = np.asfortranarray(a @ X - X * theta[None, :lowest])
        errors = np.array([O.norm(R[:, j]) for j in range(lowest)])
        eigenvalues = theta[:lowest].copy()
        eigenvectors = np.asfortranarray(X[:, :lowest])
        if policy == "all":
            has_converged |= errors < tolerance
            done = has_converged.all()
        else:
            done = (errors < tolerance).all()
        if done:
            iters = i
            break
        grow = m <= max_dim if policy == "all" else (m + lowest <= max_dim or m <= initial_dimension)
        if grow:
            if degree is None:
                T = BI.scalar_correction(a, None, theta, R)
            else:
                T = cheb_correction(a, theta, R, ncorr, lowest, degree, bound)
            if policy != "all":
                T = T[:, np.nonzero(errors >= tolerance)[0]]
            V = O.lapack_qr(O.concatenate(V, np.asfortranarray(T)))
        else:
            V = V @ Y[:, :initial_dimension]
        H = V.T @ (a @ V)
    return eigenvalues, eigenvectors, iters
