"""Shared by the tests of the Chebyshev-filtered correction with a Lanczos bound (method "LCHEB"; not collected): the test matrices, a
numpy restatement of the bound - start vector, recurrence and rule of include/davidson_hip.h, statement by statement as
fortran_davidson_amd/csrc/engine_cheb.hip makes them, only the order of the dot products is numpy's - the first coefficient of a
correction and its inverse (how a test reads the engine's bound out of a degree-1 block), and a restatement of the solve: cheb_inputs'
loop with only the bound swapped."""
import numpy as np

from oracle import davidson_oracle as O
import bdpr_inputs as BI
import cheb_inputs as CI

U = CI.U
STEPS = 12
DEFAULT_DEGREE = CI.DEFAULT_DEGREE
MAX_ITERATIONS = CI.MAX_ITERATIONS


# ---- matrices -----------------------------------------------------------------------------------------------------------------------
def stencil_matrix(n, d0, dstep, eps):
    """tests/helpers/user_operator.hip as a dense matrix: d0 + dstep * i on the diagonal, eps and eps / 2 on the first two off-diagonals"""
    a = np.diag(d0 + dstep * np.arange(n, dtype=np.float64))
    for off, w in ((1, eps), (2, 0.5 * eps)):
        a += w * (np.eye(n, k=off) + np.eye(n, k=-off))
    return a


def path_laplacian(n):
    """the Laplacian of a path: its null vector is constant, its largest eigenvalue just below 4"""
    a = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    a[0, 0] = a[-1, -1] = 1.0
    return a


def noisy_laplacian(nx=16, seed=4, sigma=1e-3):
    """the 2-D Laplacian of an nx x nx grid plus sigma x symmetric noise in every entry: a dense matrix with a nearly constant diagonal"""
    g = np.random.default_rng(seed).standard_normal((nx * nx, nx * nx))
    return CI.laplacian2d(nx) + sigma * (g + g.T) / 2.0


def bound_matrices():
    """name -> matrix: what the bound was checked on"""
    return {"lap16": CI.laplacian2d(16, 1), "lap24": CI.laplacian2d(24, 2), "block240_b4": BI.block_matrix(240, 4, 1)[0],
            "block256_b16": BI.block_matrix(256, 16, 3)[0], "random300": CI.random_sparse(300, 0.05, 7, grade=0.01),
            "random777": CI.random_sparse(777, 6.0 / 777, 777, grade=0.5 / 777), "diagonal_dominant400": O.generate_diagonal_dominant(400, 1e-3),
            "path500": path_laplacian(500)}


# name -> (matrix, lowest): the inputs of the iteration-count table
def table_inputs():
    return {"stencil300_l4": (stencil_matrix(300, 3.0, 1e-3, -1.0), 4), "stencil300_l8": (stencil_matrix(300, 3.0, 1e-3, -1.0), 8),
            "noisy_lap16_l4": (noisy_laplacian(), 4), "lap24_l8": (CI.laplacian2d(24, 2), 8),
            "block240_b4": (BI.block_matrix(240, 4, 1)[0], 4)}


# CPU restatement, policy "all", tolerance 1e-8, max_dim 10 * lowest, at most 400 iterations: name -> (DPR, LCHEB6, LCHEB10, LCHEB16)
TABLE = {
    "stencil300_l4": (203, 30, 20, 14),
    "stencil300_l8": (134, 28, 19, 14),
    "noisy_lap16_l4": (123, 18, 11, 7),
    "lap24_l8": (166, 18, 11, 7),
    "block240_b4": (56, 16, 10, 7),
}


# ---- the bound ----------------------------------------------------------------------------------------------------------------------
def start_vector(n):
    """u[g] = (splitmix64(g + 1) >> 11) * 2^-52 - 1: 53 bits in [-1, 1), exact"""
    z = O._splitmix64(np.arange(1, n + 1, dtype=np.uint64))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0


def lanczos_bound(a, steps=STEPS, product=None, trace=None):
    """b = max_i (alpha_i + beta_{i-1} + beta_i) + beta_{k-1} (beta_{k-1} left out of the last row) of k <= min(steps, n) Lanczos steps
    without reorthogonalisation from start_vector, stopped once beta <= 1e-12 max |alpha|.  The product is taken of the unnormalised
    vector and divided by its norm afterwards, as the engine does.  product: x -> A x (default a @ x)."""
    n = a.shape[0]
    prod = product or (lambda x: a @ x)
    u = start_vector(n)
    nrm, beta, amax, bound, vprev = np.sqrt(u @ u), 0.0, 0.0, 0.0, None
    k = min(steps, n)
    with np.errstate(all="ignore"):
        for i in range(k):
            au = prod(u)
            v, w = u / nrm, au / nrm
            if vprev is not None:
                w = w - beta * vprev
            alpha = float(v @ w)
            w = w - alpha * v
            before, beta = beta, float(np.sqrt(w @ w))
            amax = abs(alpha) if (abs(alpha) > amax or alpha != alpha) else amax
            last = i + 1 == k or beta <= 1e-12 * amax
            row = alpha + before if last else alpha + before + beta
            bound = row if i == 0 or row > bound or row != row else bound
            if trace is not None:
                trace.append((alpha, beta))
            if last:
                break
            nrm, vprev, u = beta, v, w
    return bound + beta


def first_coefficient(theta, ncorr, lowest, bound):
    """alpha_0 = s_1 / e of z_1 = alpha_0 r, operation by operation as cheb_coef rounds it (float64; bound may be an array); NaN where
    the interval is not usable"""
    th = np.asarray(theta[:ncorr], dtype=np.float64)
    b = np.asarray(bound, dtype=np.float64)
    a0 = th[0]
    with np.errstate(all="ignore"):
        delta = (b - a0) / 64.0
        lo = np.minimum(np.maximum(th[min(ncorr, 2 * lowest) - 1], th[lowest - 1] + delta), b - delta)
        ok = np.isfinite(b) & (b > a0) & (lo > a0) & (b > lo) & bool(np.isfinite(th).all())
        c, e = (lo + b) / 2.0, (b - lo) / 2.0
        s1 = e / (a0 - c)
        return np.where(ok, s1 / e, np.nan)


def coefficient_of_block(r, t):
    """the one double c with fl(c * r) == t bit for bit in every entry (degree 1: t = alpha_0 r), None when there is none; r, t: (n, k)"""
    r, t = np.asarray(r, dtype=np.float64), np.asarray(t, dtype=np.float64)
    i, j = np.unravel_index(np.abs(r).argmax(), r.shape)
    guess = np.array(t[i, j] / r[i, j]).view(np.int64)
    found = []
    for k in range(-8, 9):
        c = np.array(guess + k, dtype=np.int64).view(np.float64)
        if np.array_equal((c * r).view(np.uint64), t.view(np.uint64)):
            found.append(float(c))
    return found[0] if len(found) == 1 else (found or None)


def bounds_giving(alpha0, theta, ncorr, lowest, near, window=4096):
    """every double b within `window` units in the last place of `near` whose first_coefficient is alpha0 bit for bit (ascending)"""
    base = np.array(near, dtype=np.float64).view(np.int64)
    cand = (base + np.arange(-window, window + 1, dtype=np.int64)).view(np.float64)
    got = first_coefficient(theta, ncorr, lowest, cand)
    return cand[got == alpha0]


# ---- the solve ----------------------------------------------------------------------------------------------------------------------
def block_ranks(a, lowest, degree=DEFAULT_DEGREE, iterations=3):
    """[(columns, numerical rank at 1e-12)] of [V T] in the first growing iterations of restated_solve(a, lowest, "LCHEB<degree>").  Where
    the rank is below the columns the next basis depends on how the orthonormalisation completes the dependent columns - the oracle's
    Householder QR and the engine's replacement by unit vectors (davidson_ortho) differ there, and so do the iteration counts."""
    bound = lanczos_bound(a)
    V = O.generate_preconditioner(O.diagonal(a), 2 * lowest)
    out = []
    for _ in range(iterations):
        theta, Y = O.lapack_generalized_eigensolver(V.T @ (a @ V), None)
        X = V @ Y
        T = CI.cheb_correction(a, theta, a @ X - X * theta[None, :], V.shape[1], lowest, degree, bound)
        VT = np.hstack([V, T / np.linalg.norm(T, axis=0)])
        s = np.linalg.svd(VT, compute_uv=False)
        out.append((VT.shape[1], int((s > 1e-12 * s[0]).sum())))
        V = O.lapack_qr(np.asfortranarray(VT))
    return out


def method_degree(method):
    """None for "DPR", the degree of "LCHEB" / "LCHEB<d>" """
    if method == "DPR":
        return None
    assert method.startswith("LCHEB")
    return int(method[5:]) if method[5:] else DEFAULT_DEGREE


def restated_solve(a, lowest, method, policy="all", max_iterations=MAX_ITERATIONS, tolerance=1e-8):
    """cheb_inputs.restated_solve with the Lanczos bound in the place of the row sum: the oracle's dense loop (policy "all") or its
    "unconverged" variant for a standard problem, with the correction `method`: "DPR" or "LCHEB" / "LCHEB<d>".  Returns (eigenvalues,
    eigenvectors, iters)."""
    n = a.shape[0]
    degree = method_degree(method)
    bound = lanczos_bound(a)
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
                T = CI.cheb_correction(a, theta, R, ncorr, lowest, degree, bound)
            if policy != "all":
                T = T[:, np.nonzero(errors >= tolerance)[0]]
            V = O.lapack_qr(O.concatenate(V, np.asfortranarray(T)))
        else:
            V = V @ Y[:, :initial_dimension]
        H = V.T @ (a @ V)
    return eigenvalues, eigenvectors, iters
