"""Checker tool (not collected by pytest): scalar DPR against the block-diagonal correction (method "BDPR") at N = 10^6 - a block-banded
BSR matrix of b x b blocks with about 64 stored entries per row (strong coupling inside the diagonal blocks, weak hops between block
rows; given as its lower block triangle), lowest = 16, cold solves with "DPR" and "BDPR" on one engine.  Per block size and method:
iterations, block applies of A, the wall time of the solve (the solves return synchronised, so a host clock measures them) and the
time of the Ritz / residue / correction phase (davidson_engine%phase_seconds(3), host clock around the phase's calls, which end
synchronised).  The first line gives the read rate of the box (dav_bench_stream3); every BDPR line carries the byte model of one block
solve launch, 8 nloc (2 ncorr + b (1 + gev)) - the kernel's own time comes from a separate run under a kernel trace.  One JSON line
per solve on stdout.
    python tests/bdpr_sweep.py [--n 1000000] [--blocks 4,8,16] [--lowest 16] [--tol 1e-8] [--max-iterations 300]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fortran_davidson_amd as fd                                        # noqa: E402


def block_banded_lower(n, b, seed=1, per_row=64, onsite=1.0, hop=0.05):
    """(indptr, indices, data (nnzb, b, b) row-major) of the lower block triangle: block row I holds the blocks J = I - h .. I, with
    2 h + 1 = per_row / b blocks per full row (odd, at least 3); diagonal blocks symmetric with diag(0 .. b - 1) + 0.01 I on top"""
    nb = n // b
    h = max(1, (per_row // b - 1) // 2)
    rng = np.random.default_rng(seed)
    rows = np.arange(nb, dtype=np.int64)
    counts = np.minimum(rows, h) + 1
    indptr = np.zeros(nb + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    brow = np.repeat(rows, counts)
    indices = (brow - np.minimum(brow, h) + (np.arange(indptr[-1], dtype=np.int64) - indptr[brow])).astype(np.int32)
    data = rng.standard_normal((int(indptr[-1]), b, b))
    dist = brow - indices
    data *= np.where(dist == 0, onsite, hop / np.maximum(dist, 1))[:, None, None]
    d = np.flatnonzero(dist == 0)
    data[d] = (data[d] + data[d].transpose(0, 2, 1)) / 2
    ar = np.arange(b)
    data[d[:, None], ar[None, :], ar[None, :]] += ar[None, :] * 1.0 + 0.01 * brow[d][:, None]
    return indptr, indices, data, 2 * h + 1


def phase_seconds(eng):
    out = (C.c_double * 8)()
    eng.lib.fd_engine_phase_seconds(eng.p, out)
    return list(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--blocks", default="4,8,16")
    ap.add_argument("--lowest", type=int, default=16)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iterations", type=int, default=300)
    args = ap.parse_args()
    lowest = args.lowest
    for b in [int(x) for x in args.blocks.split(",")]:
        n = args.n // b * b
        indptr, indices, data, per_row = block_banded_lower(n, b)
        with fd.DavidsonEngine(n, lowest) as eng:
            if b == int(args.blocks.split(",")[0]):
                _, _, read_gbps = eng.c.bench_stream3(0, 5)
                print(json.dumps({"case": "stream", "read_GBps": round(read_gbps, 1)}), flush=True)
            eng.set_block_sparse(1, indptr, indices, data, lower=True)
            lam = {}
            for method in ("DPR", "BDPR", "DPR", "BDPR"):            # twice: the first pair pays the one-time costs
                eng.c.reset_stats()
                t0 = time.perf_counter()
                lam[method], _, iters = eng.solve(method, args.max_iterations, args.tol, want_vectors=False)
                dt = time.perf_counter() - t0
                st = eng.c.stats()
                row = {"n": n, "b": b, "blocks_per_row": per_row, "method": method, "iters": iters, "applies": st.applies,
                       "apply_cols": st.apply_cols, "wall_ms": round(1e3 * dt, 2), "correction_phase_ms": round(1e3 * phase_seconds(eng)[2], 2)}
                if method == "BDPR":
                    row["block_solve_model_bytes_at_ncorr"] = {str(k): 8 * n * (2 * k + b) for k in (2 * lowest, 4 * lowest)}
                print(json.dumps(row), flush=True)
            print(json.dumps({"n": n, "b": b, "max_eigenvalue_difference": float(np.abs(lam["DPR"] - lam["BDPR"]).max())}), flush=True)


if __name__ == "__main__":
    main()
