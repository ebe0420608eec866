"""Input families for the device eigensolver (csrc/k_smalleig.hip): projected matrices that are hard or special for a
one-workgroup cyclic Jacobi - exactly diagonal, repeated and clustered eigenvalues, graded spectra, rank deficiency,
extreme scales - and overlap matrices for the generalized path.  Plain numpy, no GPU.

Every family is a function (m, seed) -> (H, S or None); H (and S) are exactly symmetric, C-contiguous float64.
tests/test_small_eig_inputs_cpu.py checks LAPACK against 50-digit arithmetic on them, tests/test_small_eig_spectra_gpu.py
runs the kernel on them."""
import numpy as np


def _rng(m, seed):
    return np.random.default_rng(1000 * seed + m)


def _orthogonal(rng, m):
    return np.linalg.qr(rng.standard_normal((m, m)))[0]


def _sym(X):
    return 0.5 * (X + X.T)


def _similar(rng, d):
    """Q diag(d) Q^T with a random orthogonal Q, symmetrised"""
    Q = _orthogonal(rng, len(d))
    return _sym((Q * np.asarray(d, dtype=np.float64)[None, :]) @ Q.T)


# ---- standard problems -------------------------------------------------------------------------------------------------
def diagonal(m, seed=0):
    """random diagonal, not sorted"""
    return np.diag(_rng(m, seed).standard_normal(m)), None


def scaled_identity(m, seed=0):
    return 3.0 * np.eye(m), None


def zero(m, seed=0):
    return np.zeros((m, m)), None


def two_values(m, seed=0):
    """eigenvalues alternate between -2 and 1 (two eigenspaces of dimension ~m/2), dense"""
    return _similar(_rng(m, seed), np.where(np.arange(m) % 2 == 1, 1.0, -2.0)), None


def cluster(m, seed=0):
    """m//2 eigenvalues 1 + j 1e-13, the rest 2, 3, ..."""
    d = np.concatenate([1.0 + 1e-13 * np.arange(m // 2), 2.0 + np.arange(m - m // 2)])
    return _similar(_rng(m, seed), d), None


def graded_dense(m, seed=0):
    """eigenvalues logspace(-8, 6, m) under a random orthogonal similarity: graded spectrum, no graded structure"""
    return _similar(_rng(m, seed), np.logspace(-8, 6, m)), None


def graded_scaled(m, seed=0):
    """D (I + 1e-2 E) D, D = diag(logspace(-4, 3, m)), E symmetric standard normal: a well-conditioned matrix scaled
    from both sides, whose every eigenvalue is determined to high RELATIVE accuracy by the entries"""
    rng = _rng(m, seed)
    X = rng.standard_normal((m, m))
    E = np.triu(X) + np.triu(X, 1).T
    d = np.logspace(-4, 3, m)
    return (np.eye(m) + 1e-2 * E) * np.outer(d, d), None      # both factors exactly symmetric


def indefinite(m, seed=0):
    X = _rng(m, seed).standard_normal((m, m))
    return X + X.T, None


def rank_one(m, seed=0):
    q = _orthogonal(_rng(m, seed), m)[:, 0]
    return np.outer(q, q), None


def null_space(m, seed=0):
    """three eigenvalues exactly 0 by construction (a sum of m - 3 rank-one terms), the rest 1 .. m-3"""
    Q = _orthogonal(_rng(m, seed), m)[:, :max(m - 3, 0)]
    return _sym((Q * np.arange(1.0, Q.shape[1] + 1)[None, :]) @ Q.T), None


def scaled_down(m, seed=0):
    return 1e-100 * indefinite(m, seed)[0], None


def scaled_up(m, seed=0):
    return 1e+100 * indefinite(m, seed)[0], None


def wilkinson(m, seed=0):
    """tridiagonal |i - (m-1)/2| with unit off-diagonals: pairs of eigenvalues that agree to many digits"""
    H = np.diag(np.abs(np.arange(m) - (m - 1) / 2.0))
    if m > 1:
        H += np.diag(np.ones(m - 1), 1) + np.diag(np.ones(m - 1), -1)
    return H, None


# ---- generalized problems: H = indefinite ------------------------------------------------------------------------------
def S_near_identity(m, seed=0):
    X = np.random.default_rng(1000 * seed + m + 500000).standard_normal((m, m))
    return indefinite(m, seed)[0], np.eye(m) + 1e-8 * (X + X.T)


def S_cond1e10(m, seed=0):
    """overlap with eigenvalues logspace(0, -10, m): the Cholesky reduction loses digits here, in LAPACK too"""
    return indefinite(m, seed)[0], _similar(np.random.default_rng(1000 * seed + m + 600000), np.logspace(0, -10, m))


def S_late_negative(m, seed=0):
    """not positive definite, found at the LAST pivot"""
    S = np.eye(m)
    S[m - 1, m - 1] = -1.0
    return indefinite(m, seed)[0], S


def S_semidefinite(m, seed=0):
    """an exact zero pivot in the middle (pivot m//2 + 1, counted from 1)"""
    S = np.eye(m)
    S[m // 2, m // 2] = 0.0
    return indefinite(m, seed)[0], S


STANDARD = {f.__name__: f for f in (diagonal, scaled_identity, zero, two_values, cluster, graded_dense, graded_scaled, indefinite,
                                    rank_one, null_space, scaled_down, scaled_up, wilkinson)}
GENERALIZED = {f.__name__: f for f in (S_near_identity, S_cond1e10)}
NOT_POSITIVE_DEFINITE = {f.__name__: f for f in (S_late_negative, S_semidefinite)}
FAMILIES = {**STANDARD, **GENERALIZED, **NOT_POSITIVE_DEFINITE}


# ---- the measures the tests bound ---------------------------------------------------------------------------------------
def scaled_residual(H, S, theta, Y):
    """max_j ||H y_j - theta_j S y_j||_inf / ((||H||_inf + |theta_j| ||S||_inf) ||y_j||_inf), evaluated in extended
    precision so that the evaluation itself does not show at the 1e-14 level"""
    m = H.shape[0]
    Hl, Yl, tl = H.astype(np.longdouble), np.asarray(Y).astype(np.longdouble), np.asarray(theta).astype(np.longdouble)
    Sl = np.eye(m, dtype=np.longdouble) if S is None else S.astype(np.longdouble)
    R = np.abs(Hl @ Yl - (Sl @ Yl) * tl[None, :]).max(axis=0)
    nh, ns = np.abs(Hl).sum(axis=1).max(), np.abs(Sl).sum(axis=1).max()
    den = (nh + np.abs(tl) * ns) * np.abs(Yl).max(axis=0)
    den = np.maximum(den, np.longdouble(np.finfo(np.float64).tiny))
    return float((R / den).max())


def orthogonality(S, Y):
    """max |Y^T S Y - I|"""
    m = Y.shape[0]
    Yl = np.asarray(Y).astype(np.longdouble)
    Sl = np.eye(m, dtype=np.longdouble) if S is None else S.astype(np.longdouble)
    return float(np.abs(Yl.T @ Sl @ Yl - np.eye(Y.shape[1], dtype=np.longdouble)).max())
