"""Shared by the tests of the block-diagonal preconditioned correction (method "BDPR"; not collected): the block-structured test
matrices, their BSR arrays, a numpy elimination with the kernel's pivot rule and its growth factor, and a restatement of the solve - the
oracle's dense loop (oracle/davidson_oracle.py: generalized_eigensolver_dense) with only the correction swapped."""
import numpy as np

from oracle import davidson_oracle as O

U = 2.0 ** -53

# CPU restatement, lowest 4, tolerance 1e-8: (n, b, generalized, seed) -> iterations of scalar DPR and of BDPR
TABLE = {(240, 4, False, 1): (56, 22), (240, 4, False, 2): (50, 22), (240, 4, False, 3): (46, 23),
         (240, 8, False, 1): (46, 24), (240, 8, False, 2): (38, 18), (240, 8, False, 3): (50, 24),
         (256, 16, False, 1): (58, 23), (256, 16, False, 2): (46, 22), (256, 16, False, 3): (51, 20),
         (240, 4, True, 1): (58, 23), (240, 4, True, 2): (35, 19), (240, 4, True, 3): (44, 23)}


def block_matrix(n, b, seed, gev=False, onsite=1.0, hop=0.05):
    """a symmetric matrix of nb = n / b coupled b x b blocks - strong coupling inside a block, weak hops to block rows I - 1 and I - 3 -
    and (gev) an overlap matrix of the same structure around the identity"""
    rng = np.random.default_rng(seed); nb = n // b; A = np.zeros((n, n))
    for I in range(nb):
        D = rng.standard_normal((b, b)) * onsite
        A[I*b:(I+1)*b, I*b:(I+1)*b] = (D + D.T) / 2 + np.diag(np.arange(b) * 1.0 + 0.01 * I)
        for J in (I - 1, I - 3):
            if J >= 0:
                H = rng.standard_normal((b, b)) * hop
                A[I*b:(I+1)*b, J*b:(J+1)*b] = H; A[J*b:(J+1)*b, I*b:(I+1)*b] = H.T
    B = None
    if gev:
        B = np.eye(n)
        for I in range(nb):
            S = rng.standard_normal((b, b)) * 0.1; B[I*b:(I+1)*b, I*b:(I+1)*b] += (S + S.T) / 2
            if I > 0:
                H = rng.standard_normal((b, b)) * 0.01
                B[I*b:(I+1)*b, (I-1)*b:I*b] = H; B[(I-1)*b:I*b, I*b:(I+1)*b] = H.T
    return A, B


def bsr_of(a, b, lower=False, split=None, keep_diagonal=True):
    """(indptr int64, indices int32, data (nnzb, b, b) row-major blocks) of the dense symmetric matrix `a`, 0-based: every block that
    holds a non-zero (and, keep_diagonal, every diagonal block), or only those with block column <= block row.  split: a seed - every
    second diagonal block is then given as two terms (0.75 and 0.25 of it, in a seeded order among the blocks of its row): their sum
    in input order is what the operator's diagonal block is."""
    nb = a.shape[0] // b
    rng = np.random.default_rng(split) if split is not None else None
    mask = np.abs(a).reshape(nb, b, nb, b).max(axis=(1, 3)) > 0
    if keep_diagonal:
        mask |= np.eye(nb, dtype=bool)
    indptr, indices, data = [0], [], []
    for I in range(nb):
        row = []
        for J in np.flatnonzero(mask[I, :I + 1 if lower else nb]):
            blk = a[I*b:(I+1)*b, J*b:(J+1)*b]
            if I == J and rng is not None and I % 2 == 0:
                row += [(J, 0.75 * blk), (J, 0.25 * blk)]
            else:
                row.append((J, blk.copy()))
        if rng is not None:
            row = [row[i] for i in rng.permutation(len(row))]
        indices += [J for J, _ in row]
        data += [blk for _, blk in row]
        indptr.append(len(indices))
    return (np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32),
            np.ascontiguousarray(np.array(data, dtype=np.float64).reshape(-1, b, b)))


def diagonal_blocks(indptr, indices, data):
    """(nb, b, b): the diagonal blocks as the engine forms them - a block row's diagonal blocks added in input order from +0.0"""
    nb, b = len(indptr) - 1, data.shape[1]
    out = np.zeros((nb, b, b))
    for I in range(nb):
        for p in range(indptr[I], indptr[I + 1]):
            if indices[p] == I:
                out[I] += data[p]
    return out


def eliminate_batch(M, r):
    """Gaussian elimination with partial pivoting of the systems M[s] t = r[s] (M: (ns, b, b), r: (ns, b)) by the kernel's rule: the pivot
    of step k is the largest |entry| of column k among the rows not chosen yet, ties to the lowest row; rows are not swapped; a pivot
    that is exactly zero makes the solution of that system zero.  Returns (t, rho, singular): rho = max |u_ij| / max |m_ij| over every
    stage of the reduction (1 for a zero matrix)."""
    M = np.array(M, dtype=np.float64)
    r = np.array(r, dtype=np.float64)
    ns, b, _ = M.shape
    ar = np.arange(ns)
    chosen = np.zeros((ns, b), dtype=bool)
    own = np.zeros((ns, b), dtype=np.int64)
    singular = np.zeros(ns, dtype=bool)
    m0 = np.abs(M).reshape(ns, -1).max(axis=1)
    umax = m0.copy()
    with np.errstate(all="ignore"):
        for k in range(b):
            who = np.where(chosen, -1.0, np.abs(M[:, :, k])).argmax(axis=1)          # argmax: the first (lowest) among equals
            own[:, k] = who
            piv = M[ar, who, k]
            singular |= piv == 0.0
            prow, prhs = M[ar, who, :].copy(), r[ar, who].copy()
            elim = ~chosen
            elim[ar, who] = False
            f = np.where(elim, M[:, :, k] / piv[:, None], 0.0)
            M[:, :, k + 1:] = np.where(elim[:, :, None], M[:, :, k + 1:] - f[:, :, None] * prow[:, None, k + 1:], M[:, :, k + 1:])
            r = np.where(elim, r - f * prhs[:, None], r)
            chosen[ar, who] = True
            if k + 1 < b:
                rest = np.where((~chosen)[:, :, None], np.abs(M[:, :, k + 1:]), 0.0).reshape(ns, -1).max(axis=1)
                umax = np.where(singular, umax, np.maximum(umax, rest))
        t = np.zeros((ns, b))
        for k in range(b - 1, -1, -1):
            xk = r[ar, own[:, k]] / M[ar, own[:, k], k]
            r = r - M[:, :, k] * xk[:, None]
            t[:, k] = xk
    t[singular] = 0.0
    rho = np.where(m0 > 0, umax / np.where(m0 > 0, m0, 1.0), 1.0)
    return t, rho, singular


def eliminate(M, r):
    """one system: (t, rho)"""
    t, rho, _ = eliminate_batch(np.asarray(M)[None], np.asarray(r)[None])
    return t[0], float(rho[0])


def block_correction(da, db, theta, R):
    """T[I b:(I + 1) b, j] = (theta_j B_II - A_II)^-1 R[I b:(I + 1) b, j] from the diagonal blocks da, db (nb, b, b); db None: B_II = I"""
    nb, b, _ = da.shape
    m = R.shape[1]
    bI = np.broadcast_to(np.eye(b), da.shape) if db is None else db
    M = theta[:m, None, None, None] * bI[None] - da[None]                  # (m, nb, b, b)
    rhs = R.T.reshape(m, nb, b)
    t, _, _ = eliminate_batch(M.reshape(m * nb, b, b), rhs.reshape(m * nb, b))
    return np.asfortranarray(t.reshape(m, nb * b).T)


def scalar_correction(A, B, theta, R):
    """scalar DPR as the engine guards it: den != 0 ? r / den : 0"""
    da = np.diag(A)[:, None]
    th = np.asarray(theta)[None, :R.shape[1]]
    den = th * np.diag(B)[:, None] - da if B is not None else th - da
    with np.errstate(all="ignore"):
        return np.where(den != 0.0, R / den, 0.0)


def restated_solve(A, B, b, lowest, method, max_iterations=300, tolerance=1e-8):
    """generalized_eigensolver_dense of the oracle, statement by statement, with the correction `method`: "DPR" (scalar, guarded) or
    "BDPR" (the block solve on the b x b diagonal blocks).  Returns (eigenvalues, eigenvectors, iters)."""
    n = A.shape[0]
    gev = B is not None
    initial_dimension, max_dim = 2 * lowest, 10 * lowest
    has_converged = np.zeros(lowest, dtype=bool)
    nb = n // b
    da = np.stack([A[I*b:(I+1)*b, I*b:(I+1)*b] for I in range(nb)])
    db = np.stack([B[I*b:(I+1)*b, I*b:(I+1)*b] for I in range(nb)]) if gev else None
    V = O.generate_preconditioner(O.diagonal(A), initial_dimension)
    H = V.T @ (A @ V)
    S = V.T @ (B @ V) if gev else None
    eigenvalues, eigenvectors, iters = np.zeros(lowest), np.zeros((n, lowest), order="F"), max_iterations + 1
    for i in range(1, max_iterations + 1):
        theta, Y = O.lapack_generalized_eigensolver(H, S)
        X = V @ Y
        m = V.shape[1]
        R = np.empty((n, m), order="F")
        for j in range(m):
            R[:, j] = A @ X[:, j] - (theta[j] * (B @ X[:, j]) if gev else theta[j] * X[:, j])
        errors = np.array([O.norm(R[:, j]) for j in range(lowest)])
        has_converged |= errors < tolerance
        eigenvalues = theta[:lowest].copy()
        eigenvectors = np.asfortranarray(X[:, :lowest])
        if has_converged.all():
            iters = i
            break
        if m <= max_dim:
            T = block_correction(da, db, theta, R) if method == "BDPR" else scalar_correction(A, B, theta, R)
            V = O.lapack_qr(O.concatenate(V, T))
        else:
            V = V @ Y[:, :initial_dimension]
        H = V.T @ (A @ V)
        if gev:
            S = V.T @ (B @ V)
    return eigenvalues, eigenvectors, iters
