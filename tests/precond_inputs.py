"""Shared by the tests of the preconditioner slot (DAV_OP_M; not collected): the test matrices - a 2-D Laplacian plus a potential, a
sparse diagonally dominant SPD B - the builders of M as CSR, BSR, DIA and as a dense inverse written as full CSR, the integer-valued
M of the exact tests, and a numpy restatement of the solve: the oracle's dense loop (oracle/davidson_oracle.py:
generalized_eigensolver_dense) with only the correction swapped, T = M R in place of T = R / (theta dB - dA)."""
import numpy as np

from oracle import davidson_oracle as O

TOLERANCE = 1e-8
MAX_ITERATIONS = 400


# ---- matrices -----------------------------------------------------------------------------------------------------------------------
def laplacian(nx, ny):
    """the 5-point Laplacian of an nx x ny grid (Dirichlet), dense"""
    n = nx * ny
    a = np.zeros((n, n))
    for i in range(nx):
        for j in range(ny):
            p = i * ny + j
            a[p, p] = 4.0
            if j + 1 < ny:
                a[p, p + 1] = a[p + 1, p] = -1.0
            if i + 1 < nx:
                a[p, p + ny] = a[p + ny, p] = -1.0
    return a


def potential(n, scale, seed):
    return scale * np.random.default_rng(seed).random(n)


def hamiltonian(nx, ny, scale, seed):
    """(A = L + diag(v), L, v)"""
    lap = laplacian(nx, ny)
    v = potential(nx * ny, scale, seed)
    return lap + np.diag(v), lap, v


def mass_matrix(n, seed, per_row=3, weight=0.05):
    """a sparse, strictly diagonally dominant, symmetric positive definite B: unit diagonal plus about per_row off-diagonal entries
    per row of magnitude below weight (row sums of the off-diagonal part stay below 2 per_row weight < 1)"""
    rng = np.random.default_rng(seed)
    b = np.zeros((n, n))
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.integers(0, n, rows.size)
    keep = rows != cols
    b[rows[keep], cols[keep]] = weight * (2.0 * rng.random(int(keep.sum())) - 1.0)
    b = np.tril(b, -1)
    b = b + b.T
    b[np.arange(n), np.arange(n)] = 1.0
    return b


def shifted_inverse(lap, v):
    """M = inv(L + mean(v) I): the kinetic part inverted at the mean of the potential, symmetric positive definite"""
    m = np.linalg.inv(lap + np.mean(v) * np.eye(lap.shape[0]))
    return 0.5 * (m + m.T)


def stencil_matrix(n, d0, dstep, eps):
    """the matrix tests/helpers/user_operator.hip applies"""
    a = np.diag(d0 + dstep * np.arange(n, dtype=np.float64))
    for off, w in ((1, eps), (2, 0.5 * eps)):
        a += w * (np.eye(n, k=off) + np.eye(n, k=-off))
    return a


def eigh_lowest(a, b, lowest):
    """the lowest eigenvalues of A x = lambda B x by numpy.linalg.eigh (generalized: on inv(L) A inv(L)^T, B = L L^T)"""
    if b is None:
        return np.linalg.eigh(a)[0][:lowest]
    li = np.linalg.inv(np.linalg.cholesky(b))
    c = li @ a @ li.T
    return np.linalg.eigh(0.5 * (c + c.T))[0][:lowest]


def residual_norms(a, b, lam, x):
    bx = x if b is None else b @ x
    return np.linalg.norm(a @ x - bx * lam[None, :], axis=0)


# the solve cases of the GPU tests: name -> (nx, ny, potential scale, seed, lowest, generalized)
SOLVE_CASES = {"n400_std": (20, 20, 0.5, 11, 4, False), "n400_gev": (20, 20, 0.5, 12, 4, True)}
_CASES = {}


def solve_case(name):
    """(A, B | None, M, lowest) of a solve case, built once"""
    if name not in _CASES:
        nx, ny, scale, seed, lowest, gev = SOLVE_CASES[name]
        a, lap, v = hamiltonian(nx, ny, scale, seed)
        b = mass_matrix(nx * ny, seed + 100) if gev else None
        _CASES[name] = (a, b, shifted_inverse(lap, v), lowest)
    return _CASES[name]


# ---- M in the forms the engine takes ------------------------------------------------------------------------------------------------
def csr_of(a, full=False):
    """(indptr int64, indices int32, data) of the non-zeros of the dense matrix a - full: of every entry (a dense inverse as CSR)"""
    mask = np.ones(a.shape, dtype=bool) if full else a != 0.0
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(mask)
    return indptr, cols.astype(np.int32), np.ascontiguousarray(a[rows, cols], dtype=np.float64)


def bsr_of(a, b):
    """(indptr int64, indices int32, data (nnzb, b, b) row-major blocks) of the b x b blocks of a that hold a non-zero"""
    n = a.shape[0]
    assert n % b == 0
    nb = n // b
    blocks = a.reshape(nb, b, nb, b).transpose(0, 2, 1, 3)
    mask = (blocks != 0.0).any(axis=(2, 3))
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(mask)
    return indptr, cols.astype(np.int32), np.ascontiguousarray(blocks[rows, cols], dtype=np.float64)


def int_banded(n, seed, offsets=(1, 2, 5, 16), amax=7):
    """a symmetric matrix of integers |m_ij| <= amax on the diagonal and the bands `offsets` (those below n), dense: the M of the exact
    tests - with integer blocks below 2^33 in magnitude every partial sum of M R is an integer below 2^53, so any order of summation
    returns the integer product bit for bit"""
    rng = np.random.default_rng(seed)
    a = np.diag(rng.integers(1, amax + 1, n).astype(np.float64))
    for off in offsets:
        if off < n:
            w = rng.integers(-amax, amax + 1, n - off).astype(np.float64)
            a += np.diag(w, off) + np.diag(w, -off)
    return a


# ---- the solve ----------------------------------------------------------------------------------------------------------------------
def scalar_correction(a, b, theta, r):
    """T = R / (theta_j dB_i - dA_i), 0 where the denominator is: DPR as the engine guards it"""
    da = np.diag(a)[:, None]
    db = np.diag(b)[:, None] if b is not None else 1.0
    den = theta[None, :r.shape[1]] * db - da
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0.0, r / den, 0.0)


def restated_solve(a, lowest, b=None, m=None, max_iterations=MAX_ITERATIONS, tolerance=TOLERANCE):
    """generalized_eigensolver_dense of the oracle (the reference's policy: one correction per basis vector, sticky convergence flags,
    collapse to 2 lowest columns above 10 lowest), statement by statement, with the DPR correction (m None) or T = M R.
    Returns (eigenvalues, eigenvectors, iters); iters = max_iterations + 1: not converged."""
    n = a.shape[0]
    initial_dimension, max_dim = 2 * lowest, 10 * lowest
    has_converged = np.zeros(lowest, dtype=bool)
    V = O.generate_preconditioner(O.diagonal(a), initial_dimension)
    H = V.T @ (a @ V)
    S = V.T @ (b @ V) if b is not None else None
    eigenvalues, eigenvectors, iters = np.zeros(lowest), np.zeros((n, lowest), order="F"), max_iterations + 1
    for i in range(1, max_iterations + 1):
        theta, Y = O.lapack_generalized_eigensolver(H, S)
        X = V @ Y
        R = np.asfortranarray(a @ X - (X if b is None else b @ X) * theta[None, :])
        errors = np.array([O.norm(R[:, j]) for j in range(lowest)])
        has_converged |= errors < tolerance
        eigenvalues = theta[:lowest].copy()
        eigenvectors = np.asfortranarray(X[:, :lowest])
        if has_converged.all():
            iters = i
            break
        if V.shape[1] <= max_dim:
            T = scalar_correction(a, b, theta, R) if m is None else m @ R
            V = O.lapack_qr(O.concatenate(V, np.asfortranarray(T)))
        else:
            V = V @ Y[:, :initial_dimension]
        H = V.T @ (a @ V)
        if b is not None:
            S = V.T @ (b @ V)
    return eigenvalues, eigenvectors, iters
