"""Checker tool (not collected by pytest): the re-solve loop with and without warm starts at N = 10^6 - a banded CSR matrix (65 entries
per row), lowest = 16, DPR; ten steps of "new values on the kept pattern (a symmetric relative perturbation of --eps), then solve", once
cold every step and once with reuse_vectors, on two engines in the same process.  Per step and mode: iterations, block applies of A and
the wall time of the solve (the solves return synchronised, so a host clock measures them).  The first line gives the read rate of the
box (dav_bench_stream3) and the byte model of one ingest of a 2 * lowest column guess (16 nloc ncols: 8 read + 8 written) together with
the wall time of dav_set_guess_dev for it - the ingest kernel's own time comes from a separate run under a kernel trace.  One JSON line
per step on stdout.
    python tests/guess_sweep.py [--n 1000000] [--lowest 16] [--steps 10] [--eps 1e-3] [--tol 1e-8]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fortran_davidson_amd as fd                                        # noqa: E402
from sparse_apply_sweep import banded                                    # noqa: E402


def symmetric_perturbation(indptr, cols, vals, eps, step):
    """vals (1 + eps u) with u in [-1, 1] a function of the unordered pair (row, column) and the step: the matrix stays symmetric"""
    n = indptr.size - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    lo, hi = np.minimum(rows, cols).astype(np.uint64), np.maximum(rows, cols).astype(np.uint64)
    with np.errstate(over="ignore"):                         # (wrapping 64-bit products are the hash)
        h = lo * np.uint64(0x9E3779B97F4A7C15) + hi * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(step) * np.uint64(0x165667B19E3779F9)
    h = (h >> np.uint64(16)) & np.uint64(0xFFFFFFFFFFFF)
    return vals * (1.0 + eps * (h.astype(np.float64) / float(0xFFFFFFFFFFFF) * 2.0 - 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--lowest", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--tol", type=float, default=1e-8)
    args = ap.parse_args()
    n, lowest = args.n, args.lowest
    indptr, cols, vals = banded(n)
    with fd.DavidsonEngine(n, lowest) as cold, fd.DavidsonEngine(n, lowest) as warm:
        _, _, read_gbps = cold.c.bench_stream3(0, 5)
        guess = torch.randn((2 * lowest, n), dtype=torch.float64, device="cuda:0").t()
        t0 = time.perf_counter()
        cold.c.set_guess(guess)
        ingest_s = time.perf_counter() - t0
        cold.c.panel_put(3, 0, np.zeros((n, 1)))             # X rewritten: nothing stays staged on the cold engine
        print(json.dumps({"case": "stream", "read_GBps": round(read_gbps, 1), "ingest_columns": 2 * lowest,
                          "ingest_model_bytes": 16 * n * 2 * lowest, "set_guess_dev_wall_ms": round(1e3 * ingest_s, 3)}), flush=True)
        for eng in (cold, warm):
            eng.set_sparse(1, indptr, cols, vals, keep_map=True)
        warm.keep_result_as_guess(True)
        for step in range(args.steps + 1):                   # step 0: the unperturbed matrix, cold on both engines
            v = vals if step == 0 else symmetric_perturbation(indptr, cols.astype(np.int64), vals, args.eps, step)
            row = {"step": step}
            lam = {}
            for name, eng in (("cold", cold), ("warm", warm)):
                if step > 0:
                    eng.update_values(1, v)
                eng.c.reset_stats()
                staged = eng.c.guess_columns()
                t0 = time.perf_counter()
                lam[name], _, iters = eng.solve("DPR", 1000, args.tol, want_vectors=False)
                dt = time.perf_counter() - t0
                st = eng.c.stats()
                row[name] = {"staged": staged, "iters": iters, "applies": st.applies, "apply_cols": st.apply_cols, "wall_ms": round(1e3 * dt, 2)}
            row["max_eigenvalue_difference"] = float(np.abs(lam["cold"] - lam["warm"]).max())
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
