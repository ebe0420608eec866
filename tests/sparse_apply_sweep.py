"""Checker tool (not collected by pytest): the CSR block product (dav_set_operator_csr, fortran_davidson_amd/csrc/k_spmm.hip) measured at
N = 10^6 for k = 8, 16, 32, 64 on three matrix classes - banded (65 nonzeros per row), uniformly random columns (64 per row), and skewed
(power-law row lengths with the same mean plus one arrowhead row holding all N entries) - with dav_bench_apply2 (ms end to end, kernel
ms, bytes of the model 12 nnz + 8 (nloc + 1) + 8 N k + 8 nloc k) against the read rate of the same box (dav_bench_stream3).  Then a full
solve of the banded case (lowest 16, DPR) and the N = 20000 CSR-versus-dense comparison of tests/test_sparse_gpu.py.  One JSON line per
case on stdout.

    python tests/sparse_apply_sweep.py [--reps 20] [--quick]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import fortran_davidson_amd as fd            # noqa: E402
from fortran_davidson_amd.engine_c import OP_A  # noqa: E402

HBM_PEAK_GBPS = 8000.0


def banded(n, half=32):
    counts = np.minimum(np.arange(n), half) + 1 + np.minimum(n - 1 - np.arange(n), half)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    rows = np.repeat(np.arange(n, dtype=np.int64), counts)
    first = np.maximum(np.arange(n, dtype=np.int64) - half, 0)
    cols = (first[rows] + (np.arange(indptr[-1], dtype=np.int64) - indptr[rows])).astype(np.int32)
    d = np.abs(cols - rows)
    vals = np.where(d == 0, 1.0 + rows.astype(np.float64), 1e-2 / (1.0 + d))
    return indptr, cols, vals


def by_lengths(n, counts, rng):
    """rows of the given lengths, uniformly random columns sorted within each row, the diagonal first"""
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    cols = rng.integers(0, n, int(indptr[-1]), dtype=np.int32)
    cols[indptr[:-1][counts > 0]] = np.arange(n, dtype=np.int32)[counts > 0]
    vals = rng.uniform(0.0, 1e-3, cols.size)
    vals[indptr[:-1][counts > 0]] = 1.0 + np.arange(n)[counts > 0]
    return indptr, cols, vals


def uniform(n, rng, per_row=64):
    return by_lengths(n, np.full(n, per_row, dtype=np.int64), rng)


def skewed(n, rng, mean=64):
    """power-law row lengths (Pareto, shape 1.5) scaled to the mean, clipped to [1, n]; row 0 holds all n entries"""
    raw = rng.pareto(1.5, n) + 1.0
    counts = np.clip(np.rint(raw * (mean / raw.mean())), 1, n).astype(np.int64)
    counts[0] = n
    return by_lengths(n, counts, rng)


def stats(indptr):
    lens = np.diff(indptr)
    return {"nnz": int(indptr[-1]), "row_len_median": float(np.median(lens)), "row_len_max": int(lens.max()),
            "rows_over_chunk": int((lens > 1024).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--quick", action="store_true", help="skip the solves")
    args = ap.parse_args()
    n = args.n
    rng = np.random.default_rng(2026)
    read_gbps = None
    for name, make in (("banded65", lambda: banded(n)), ("uniform64", lambda: uniform(n, rng)), ("skewed64", lambda: skewed(n, rng))):
        t0 = time.perf_counter()
        indptr, cols, vals = make()
        with fd.CEngine(n=n, max_cols=64) as e:
            t1 = time.perf_counter()
            e.set_operator_csr(OP_A, indptr, cols, vals)
            setup_s = time.perf_counter() - t1
            if read_gbps is None:
                _, _, read_gbps = e.bench_stream3(0, 5)
                print(json.dumps({"case": "stream", "read_GBps": round(read_gbps, 1)}), flush=True)
            for k in (8, 16, 32, 64):
                ms, kms, nbytes, flops = e.bench_apply2(k, args.reps)
                gbps = nbytes / (kms * 1e-3) / 1e9
                print(json.dumps({"case": name, "n": n, "k": k, **stats(indptr), "apply_ms": round(ms, 4), "kernel_ms": round(kms, 4),
                                  "model_bytes": nbytes, "kernel_GBps": round(gbps, 1), "frac_read_rate": round(gbps / read_gbps, 3),
                                  "frac_8TBps": round(gbps / HBM_PEAK_GBPS, 3), "GFLOPs": round(flops / (kms * 1e-3) / 1e9, 1),
                                  "setup_s": round(setup_s, 2), "build_s": round(t1 - t0, 2)}), flush=True)
        if name == "banded65" and not args.quick:
            t0 = time.perf_counter()
            with fd.DavidsonEngine(n, 16) as eng:
                eng.set_sparse(1, indptr, cols, vals)
                t1 = time.perf_counter()
                lam, _, it = eng.solve("DPR", 100, 1e-8, want_vectors=False)
                t2 = time.perf_counter()
                st = eng.c.stats()
            print(json.dumps({"case": "solve_banded65", "n": n, "lowest": 16, "method": "DPR", "iters": it, "set_s": round(t1 - t0, 2),
                              "solve_s": round(t2 - t1, 3), "applies": st.applies, "apply_ms": round(st.apply_ms, 3),
                              "lambda_0": float(lam[0])}), flush=True)
        del indptr, cols, vals
    if not args.quick:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from test_sparse_gpu import coo_to_csr, dense_of, sparse_dd
        n2, lowest = 20000, 8
        r, c, v = sparse_dd(n2, 31, per_row=100)
        out = {"case": "csr_vs_dense", "n": n2, "lowest": lowest, "nnz": int(r.size)}
        for label in ("csr", "dense"):
            with fd.DavidsonEngine(n2, lowest) as eng:
                t0 = time.perf_counter()
                if label == "csr":
                    eng.set_sparse(1, *coo_to_csr(n2, r, c, v))
                else:
                    eng.set_dense(1, dense_of(n2, r, c, v))
                t1 = time.perf_counter()
                lam, _, it = eng.solve("DPR", 200, 1e-8, want_vectors=False)
                t2 = time.perf_counter()
                st = eng.c.stats()
                k16 = eng.c.bench_apply2(16, args.reps)
            out[label] = {"iters": it, "set_s": round(t1 - t0, 3), "solve_s": round(t2 - t1, 4), "apply_ms_total": round(st.apply_ms, 3),
                          "apply16_ms": round(k16[0], 4), "apply16_kernel_ms": round(k16[1], 4), "lambda": [float(x) for x in lam]}
        out["max_lambda_diff"] = float(np.abs(np.array(out["csr"]["lambda"]) - np.array(out["dense"]["lambda"])).max())
        for label in ("csr", "dense"):
            del out[label]["lambda"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
