"""Shared by the tests of the built block preconditioner (davq_build_block_fsai, include/davidson_hip_bprecond.h; not collected): the
canonical block store of a BSR input as the engine keeps it, its expansion to CSR with every entry of every stored block kept, the block
pattern (fsai_inputs.pattern on the block index arrays), a numpy restatement of the block row in the kernel's order - the gather summing
duplicate blocks from +0.0 in stored order, the Cholesky factorisation column by column, the b back substitutions of L^T X = E from the
last row up - and a reference by numpy.linalg.solve that owes nothing to it: scalar row t of block row I is y / sqrt(y_k) with
C[:k, :k] y = e_k, k = s - b + t + 1, which is fsai_inputs.reference_rows on the scalar pattern of the expanded matrix.  The bound per
scalar row is that of DESIGN section 29 with the order k of the system solved: 8 k^2 eps cond_2(C[:k, :k]) ||g_ref||_2."""
import numpy as np

import fsai_inputs as F
import herm_inputs as H
import precond_inputs as P

MAX_COLS = 64          # BFSAI_MAX_COLS of csrc/kernels.h
cached = F.cached


# ---- stores -----------------------------------------------------------------------------------------------------------------------------
def canonical_blocks(indptr, indices, blocks, lower=False):
    """the canonical block store the engine keeps of a BSR input with row-major blocks (one rank): every block row its own blocks in input
    order, then (lower) the mirrored strict lower blocks, transposed, in the order of their source rows, stably sorted by block column"""
    nb = indptr.size - 1
    rows = np.repeat(np.arange(nb), np.diff(indptr))
    cols = np.asarray(indices, dtype=np.int64)
    vals = np.asarray(blocks, dtype=np.float64)
    if lower:
        strict = cols < rows
        rows, cols, vals = (np.concatenate([rows, cols[strict]]), np.concatenate([cols, rows[strict]]),
                            np.concatenate([vals, vals[strict].transpose(0, 2, 1)]))
    order = np.lexsort((np.arange(rows.size), cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nb))]).astype(np.int64)
    return rp, cols.astype(np.int32), np.ascontiguousarray(vals)


def expanded(store):
    """the canonical CSR store of the same matrix, every entry of every stored block kept (zeros too), duplicates in stored order"""
    rp, ci, vals = store
    nb, b = rp.size - 1, vals.shape[1] if vals.size else 1
    brow = np.repeat(np.arange(nb), np.diff(rp))
    rows = (brow[:, None, None] * b + np.arange(b)[None, :, None] + np.zeros((1, 1, b), dtype=np.int64)).ravel()
    cols = (ci.astype(np.int64)[:, None, None] * b + np.zeros((1, b, 1), dtype=np.int64) + np.arange(b)[None, None, :]).ravel()
    data = vals.ravel()
    order = np.lexsort((np.arange(rows.size), rows))          # by scalar row, blocks in stored order
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nb * b))]).astype(np.int64)
    return F.canonical(indptr, cols[order].astype(np.int32), np.ascontiguousarray(data[order]))


def expanded_of(store):
    """expanded(store), built once per store (the store's values are held, so their id stays theirs)"""
    return cached(("expanded", id(store[2])), lambda: (store[2], expanded(store)))[1]


def expanded_input(indptr, indices, blocks):
    """the CSR arrays of a FULL BSR input for dav_set_operator_csr: every entry of every stored block"""
    return expanded(canonical_blocks(indptr, indices, blocks))


def block_pattern(store, level):
    """(indptr, indices) of P_level over the block rows: fsai_inputs.pattern on the block index arrays"""
    return F.pattern((store[0], store[1], None), level)


def scalar_pattern(bpat, b):
    """the scalar pattern of the block pattern: row I b + t holds the columns J_q b + r of block row I up to its own, k = s - b + t + 1"""
    rp, ci = bpat
    rows = []
    for i in range(rp.size - 1):
        cols = (ci[rp[i]:rp[i + 1]].astype(np.int64)[:, None] * b + np.arange(b)[None, :]).ravel()
        for t in range(b):
            rows.append(cols[:cols.size - b + t + 1])
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, dtype=np.int32)


def scalar_rows(bpat, b, gblocks):
    """the values of the scalar rows of G on scalar_pattern(bpat, b), from its blocks gblocks (nnzb, b, b) row-major"""
    rp = bpat[0]
    out = []
    for i in range(rp.size - 1):
        blk = gblocks[rp[i]:rp[i + 1]]                       # (m, t, r)
        flat = blk.transpose(1, 0, 2).reshape(b, -1)          # row t: (q, r) ascending
        for t in range(b):
            out.append(flat[t, :flat.shape[1] - b + t + 1])
    return np.concatenate(out) if out else np.zeros(0)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def block_row_of_g(c, b):
    """the block row of G from the gathered C (order s = m b) in the kernel's order: (m, b, b) row-major blocks, or None where a pivot is
    not finite or not > 0"""
    s = c.shape[0]
    low = np.tril(c).copy()
    for k in range(s):
        d = low[k, k]
        if not (d > 0.0) or not np.isfinite(d):
            return None
        piv = np.sqrt(d)
        low[k + 1:, k] = low[k + 1:, k] / piv
        low[k, k] = piv
        col = low[k + 1:, k]
        low[k + 1:, k + 1:] -= np.tril(np.outer(col, col))
    x = np.zeros((s, b))
    x[s - b + np.arange(b), np.arange(b)] = 1.0
    for p in range(s - 1, -1, -1):
        live = p <= s - b + np.arange(b)                      # column t has nothing above its own row
        x[p, live] = x[p, live] / low[p, p]
        x[:p, live] -= low[p, :p, None] * x[p, live][None, :]
    g = x.reshape(s // b, b, b).transpose(0, 2, 1).copy()     # block q: [t][r] = X[q b + r][t]
    g[-1] = np.tril(g[-1]) + 0.0
    return g


def bfsai_rows(a, bm, sigma, level, bpat=None):
    """(indptr, indices, blocks (nnzb, b, b), first_bad) of G on block_pattern(a, level) of the canonical block store a; bm: the
    canonical block store of B or None (the identity); first_bad = the smallest block row with a failed pivot (its blocks NaN) or None"""
    b = a[2].shape[1]
    rp, ci = block_pattern(a, level) if bpat is None else bpat
    ea, eb = expanded_of(a), None if bm is None else expanded_of(bm)
    out = np.full((ci.size, b, b), np.nan)
    first_bad = None
    for i in range(rp.size - 1):
        cols = (ci[rp[i]:rp[i + 1]].astype(np.int64)[:, None] * b + np.arange(b)[None, :]).ravel()
        g = block_row_of_g(F.gathered(ea, eb, sigma, cols), b)
        if g is None:
            first_bad = i if first_bad is None else first_bad
        else:
            out[rp[i]:rp[i + 1]] = g
    return rp, ci, out, first_bad


def reference(a, bm, sigma, bpat):
    """(scalar pattern, reference values, cond_2 per scalar row) by numpy.linalg.solve on the expanded columns"""
    b = a[2].shape[1]
    spat = scalar_pattern(bpat, b)
    ref, conds = F.reference_rows(expanded_of(a), None if bm is None else expanded_of(bm), sigma, spat)
    return spat, ref, conds


def dense_factor(n, rp, ci, blocks):
    b = blocks.shape[1]
    g = np.zeros((n, n))
    for i in range(rp.size - 1):
        for p in range(rp[i], rp[i + 1]):
            g[i * b:(i + 1) * b, ci[p] * b:(ci[p] + 1) * b] = blocks[p]
    return g


def transpose_bsr(nb, rp, ci, blocks):
    """the BSR arrays of G^T, block rows ascending in the block column, every block transposed (G holds no duplicates: the order is unique)"""
    rows = np.repeat(np.arange(nb), np.diff(rp))
    order = np.lexsort((rows, ci))
    trp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=nb))]).astype(np.int64)
    return trp, rows[order].astype(np.int32), np.ascontiguousarray(blocks[order].transpose(0, 2, 1))


def dense_of(store, n):
    """the dense matrix of a canonical block store (duplicates summed)"""
    rp, ci, vals = store
    b = vals.shape[1]
    a = np.zeros((n, n))
    for i in range(rp.size - 1):
        for p in range(rp[i], rp[i + 1]):
            a[i * b:(i + 1) * b, ci[p] * b:(ci[p] + 1) * b] += vals[p]
    return a


def bsr_of_mask(a, b, mask):
    """(indptr, indices, blocks) of the b x b blocks of the dense a where mask (nb x nb) is set: every such block stored whole"""
    nb = a.shape[0] // b
    blocks = a.reshape(nb, b, nb, b).transpose(0, 2, 1, 3)
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(mask)
    return indptr, cols.astype(np.int32), np.ascontiguousarray(blocks[rows, cols], dtype=np.float64)


# ---- (a) the block-banded matrix --------------------------------------------------------------------------------------------------------
BLOCK_SIZES = (1, 2, 3, 4, 8, 16)


def half_bandwidth(b):
    return MAX_COLS // b - 1


def banded_sizes(b):
    """the block orders of the banded case: 1, 5 and one above twice the bandwidth"""
    return (1, 5, 2 * half_bandwidth(b) + 3)


def lower_with_split_blocks(indptr, indices, blocks, seed=7, every=5):
    """the lower block triangle of a full BSR input (DAV_CSR_LOWER), every `every`-th block split into two terms v = t + (v - t) that
    follow each other: duplicate blocks, separate terms in stored order"""
    rng = np.random.default_rng(seed)
    rp, ci, vv = [0], [], []
    count = 0
    for i in range(indptr.size - 1):
        for p in range(indptr[i], indptr[i + 1]):
            if indices[p] > i:
                continue
            count += 1
            if count % every == 0:
                t = blocks[p] * rng.random(blocks[p].shape)
                ci += [indices[p], indices[p]]
                vv += [t, blocks[p] - t]
            else:
                ci.append(indices[p])
                vv.append(blocks[p])
        rp.append(len(ci))
    return np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.ascontiguousarray(np.array(vv, dtype=np.float64))


def banded_case(b, nb):
    """(full BSR input, lower input with split blocks) of the block-banded SPD matrix: dense blocks inside the block half-bandwidth
    64 // b - 1, off-diagonal entries uniform in (-1, 1), diagonal = row sum of |a_ij| + 1 + rand"""
    def make():
        rng = np.random.default_rng(100 * b + nb)
        n, hb = nb * b, half_bandwidth(b)
        bi = np.arange(n) // b
        mask = np.abs(bi[:, None] - bi[None, :]) <= hb
        a = np.where(mask, 2.0 * rng.random((n, n)) - 1.0, 0.0)
        a = np.tril(a, -1)
        a = a + a.T
        a[np.arange(n), np.arange(n)] = np.abs(a).sum(axis=1) + 1.0 + rng.random(n)
        bmask = np.abs(np.arange(nb)[:, None] - np.arange(nb)[None, :]) <= hb
        full = bsr_of_mask(a, b, bmask)
        return full, lower_with_split_blocks(*full)
    return cached(("banded", b, nb), make)


def banded_refusal(b):
    """a block band of 65 // b + 1 blocks: block row 64 // b, of 64 // b + 1 blocks, is the first with more than 64 scalar columns"""
    nb, hb = 65 // b + 3, 65 // b
    n = nb * b
    a = np.full((n, n), -0.01)
    a[np.arange(n), np.arange(n)] = 2.0
    bmask = np.abs(np.arange(nb)[:, None] - np.arange(nb)[None, :]) <= hb
    return bsr_of_mask(a, b, bmask)


# ---- (b) the multi-orbital grid pencil ----------------------------------------------------------------------------------------------------
def multi_orbital(nx, ny, b, gev, seed=21):
    """(A dense, B dense | None, block mask, sigma): b orbitals per site of an nx x ny grid - kron(L, I_b), a weak inter-orbital hop
    between neighbouring sites, random symmetric on-site blocks; B = I plus a weak symmetric overlap on the same blocks; sigma =
    lambda_min - 0.3"""
    def make():
        rng = np.random.default_rng(seed + 1000 * b + nx * ny)
        nsite = nx * ny
        lap = P.laplacian(nx, ny)
        adj = (lap == -1.0).astype(np.float64)
        w = rng.standard_normal((b, b))
        hop = 0.1 * (w + w.T) / 2
        a = np.kron(lap, np.eye(b)) + np.kron(adj, hop)
        for s in range(nsite):
            v = rng.standard_normal((b, b))
            a[s * b:(s + 1) * b, s * b:(s + 1) * b] += 0.5 * (v + v.T) / 2 + np.diag(0.5 * rng.random(b))
        bm = None
        if gev:
            u = rng.standard_normal((b, b))
            bm = np.eye(nsite * b) + np.kron(adj, 0.03 * (u + u.T) / 2)
            for s in range(nsite):
                v = rng.standard_normal((b, b))
                bm[s * b:(s + 1) * b, s * b:(s + 1) * b] += 0.04 * (v + v.T) / 2
        mask = lap != 0.0
        sigma = float(P.eigh_lowest(a, bm, 1)[0]) - 0.3
        return a, bm, mask, sigma
    return cached(("orbital", nx, ny, b, gev, seed), make)


def orbital_stores(nx, ny, b, gev):
    """(BSR input of A, BSR input of B | None) of the multi-orbital case"""
    a, bm, mask, _ = multi_orbital(nx, ny, b, gev)
    return bsr_of_mask(a, b, mask), None if bm is None else bsr_of_mask(bm, b, mask)


# ---- (c) the Peierls lattice in real form --------------------------------------------------------------------------------------------------
def peierls(gev, nx=12):
    """(H, S | None, CSR arrays of H, of S | None) of herm_inputs.fortran_matrix / fortran_overlap"""
    def make():
        h = H.fortran_matrix(nx)
        s = H.fortran_overlap(nx) if gev else None
        return h, s, H.dense_csr(h), None if s is None else H.dense_csr(s)
    return cached(("peierls", gev, nx), make)


def peierls_stores(gev):
    """(BSR input of the real form of H, of S | None): the blocks [[re, -im], [im, re]] the Hermitian entry builds"""
    _, _, hc, sc = peierls(gev)
    as_bsr = lambda m: (m[0], m[1].astype(np.int32), H.expand_blocks(m[2]))          # noqa: E731
    return as_bsr(hc), None if sc is None else as_bsr(sc)


# ---- (d) the block arrow --------------------------------------------------------------------------------------------------------------------
def arrow(nb=300, b=2, seed=9):
    """lower BSR input, diagonally dominant, the first block column full: block row I of G holds the blocks {0, I}, and block row 0 of
    G^T holds nb blocks - more than the chunk of the block product"""
    rng = np.random.default_rng(seed)
    rp, ci, vv = [0], [], []
    for i in range(nb):
        if i > 0:
            ci.append(0)
            vv.append((2.0 * rng.random((b, b)) - 1.0) / nb)
        d = 0.1 * (2.0 * rng.random((b, b)) - 1.0)
        ci.append(i)
        vv.append((d + d.T) / 2 + (2.0 + rng.random()) * np.eye(b))
        rp.append(len(ci))
    return np.array(rp, dtype=np.int64), np.array(ci, dtype=np.int32), np.ascontiguousarray(np.array(vv))


# ---- the solve cases of the GPU tests: name -> (A dense, B dense | None, sigma, lowest, block size, BSR inputs | Hermitian CSR arrays) ----
SOLVE_CASES = ("orbital_std", "orbital_gev", "peierls_std", "peierls_gev")
ORBITAL_SOLVE = (10, 10, 4)          # grid and orbitals of the solve cases on (b)


def solve_case(name):
    def make():
        kind, form = name.split("_")
        gev = form == "gev"
        if kind == "orbital":
            nx, ny, b = ORBITAL_SOLVE
            a, bm, _, sigma = multi_orbital(nx, ny, b, gev)
            sa, sb = orbital_stores(nx, ny, b, gev)
            return {"a": a, "b": bm, "sigma": sigma, "lowest": 4, "bs": b, "sa": sa, "sb": sb, "herm": None}
        h, s, hc, sc = peierls(gev)
        sa, sb = peierls_stores(gev)
        return {"a": H.real_form(h), "b": None if s is None else H.real_form(s), "sigma": 0.0, "lowest": 8, "bs": 2, "sa": sa, "sb": sb,
                "herm": (h, s, hc, sc)}
    return cached(("case", name), make)


def restated_m(name, level):
    """M = G^T G (dense) of a solve case from the restatement"""
    def make():
        c = solve_case(name)
        a = canonical_blocks(*c["sa"])
        bm = None if c["sb"] is None else canonical_blocks(*c["sb"])
        rp, ci, blocks, bad = bfsai_rows(a, bm, c["sigma"], level)
        assert bad is None
        g = dense_factor(c["a"].shape[0], rp, ci, blocks)
        return g.T @ g
    return cached(("M", name, level), make)


def restated_iterations(name, level=None):
    """(eigenvalues, eigenvectors, iterations) of the restated solve of a case: plain DPR (level None) or with the restated M"""
    def make():
        c = solve_case(name)
        return P.restated_solve(c["a"], c["lowest"], c["b"], None if level is None else restated_m(name, level))
    return cached(("solve", name, level), make)
