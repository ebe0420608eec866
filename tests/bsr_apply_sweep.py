"""Checker tool (not collected by pytest): the BSR block product (dav_set_operator_bsr, fortran_davidson_amd/csrc/k_bsrmm.hip) measured at
N = 10^6 for k = 8, 16, 32, 64 and b = 4, 8, 16 on two matrix classes - a block band (half-width chosen so that a row holds about 65
entries, as the CSR sweep's band) and uniformly random block columns (64 / b blocks per block row plus the diagonal block) - and the SAME
matrices through the CSR operator (dav_set_operator_csr, k_spmm.hip).  dav_bench_apply2 gives ms end to end, kernel ms and the bytes of
each operator's model (BSR: 8 nnzb b^2 + 4 nnzb + 8 (block rows + 1) + 8 N k + 8 nloc k), against the read rate of the same box
(dav_bench_stream3).  One JSON line per case on stdout.

    python tests/bsr_apply_sweep.py [--reps 20] [--n 1000000] [--bs 4,8,16]
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

HALF = {4: 8, 8: 4, 16: 2}                   # block half-widths of the band: 68 / 72 / 80 entries per row


def block_band(n, b):
    nb, half = n // b, HALF.get(b, max(1, 32 // b))
    I = np.arange(nb, dtype=np.int64)
    counts = np.minimum(I, half) + 1 + np.minimum(nb - 1 - I, half)
    indptr = np.zeros(nb + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    bi = np.repeat(I, counts)
    bj = np.maximum(I - half, 0)[bi] + (np.arange(indptr[-1], dtype=np.int64) - indptr[bi])
    r = bi[:, None, None] * b + np.arange(b)[None, :, None]
    c = bj[:, None, None] * b + np.arange(b)[None, None, :]
    d = np.abs(r - c)
    vals = np.where(d == 0, 1.0 + r.astype(np.float64), 1e-2 / (1.0 + d))
    return indptr, bj.astype(np.int32), vals


def block_uniform(n, b, rng):
    """the diagonal block first, then 64 / b uniformly random block columns (sorted) per block row"""
    nb, per = n // b, max(1, 64 // b)
    indptr = np.arange(nb + 1, dtype=np.int64) * (per + 1)
    cols = np.sort(rng.integers(0, nb, (nb, per), dtype=np.int64), axis=1)
    bj = np.concatenate([np.arange(nb, dtype=np.int64)[:, None], cols], axis=1).ravel()
    vals = rng.uniform(0.0, 1e-3, (bj.size, b, b))
    vals[::per + 1] += np.eye(b)[None] * (1.0 + np.arange(n, dtype=np.float64).reshape(nb, b))[:, :, None]
    return indptr, bj.astype(np.int32), vals


def to_csr(n, b, indptr, bj, vals):
    """the same matrix as CSR: each block row's b rows hold the b entries of each of its blocks, in block order"""
    nb = n // b
    lens = np.diff(indptr)
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.repeat(lens * b, b), out=rp[1:])
    # entry order: block row I, row m, block p of the row, column q
    bi = np.repeat(np.arange(nb, dtype=np.int64), lens)
    cols = np.empty(int(rp[-1]), dtype=np.int32)
    vv = np.empty(int(rp[-1]))
    for m in range(b):
        for q in range(b):
            # position of (row I*b + m, block p, column q): rp[I*b + m] + (p - indptr[I]) * b + q
            pos = rp[bi * b + m] + (np.arange(bj.size, dtype=np.int64) - indptr[bi]) * b + q
            cols[pos] = bj.astype(np.int64) * b + q
            vv[pos] = vals[:, m, q]
    assert nb * b == n
    return rp, cols, vv


def measure(e, k, reps, read_gbps):
    ms, kms, nbytes, flops = e.bench_apply2(k, reps)
    gbps = nbytes / (kms * 1e-3) / 1e9
    return {"apply_ms": round(ms, 4), "kernel_ms": round(kms, 4), "model_bytes": nbytes, "kernel_GBps": round(gbps, 1),
            "frac_read_rate": round(gbps / read_gbps, 3), "GFLOPs": round(flops / (kms * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--bs", default="4,8,16")
    args = ap.parse_args()
    n = args.n
    rng = np.random.default_rng(2026)
    read_gbps = None
    for b in [int(x) for x in args.bs.split(",")]:
        for name, make in (("band", lambda: block_band(n, b)), ("uniform", lambda: block_uniform(n, b, rng))):
            t0 = time.perf_counter()
            indptr, bj, vals = make()
            build_s = time.perf_counter() - t0
            res = {}
            with fd.CEngine(n=n, max_cols=64) as e:
                if read_gbps is None:
                    _, _, read_gbps = e.bench_stream3(0, 5)
                    print(json.dumps({"case": "stream", "read_GBps": round(read_gbps, 1)}), flush=True)
                t1 = time.perf_counter()
                e.set_operator_bsr(OP_A, indptr, bj, vals)
                setup_bsr = time.perf_counter() - t1
                for k in (8, 16, 32, 64):
                    res[("bsr", k)] = measure(e, k, args.reps, read_gbps)
                rp, cols, vv = to_csr(n, b, indptr, bj, vals)
                t1 = time.perf_counter()
                e.set_operator_csr(OP_A, rp, cols, vv)
                setup_csr = time.perf_counter() - t1
                del rp, cols, vv
                for k in (8, 16, 32, 64):
                    res[("csr", k)] = measure(e, k, args.reps, read_gbps)
            for k in (8, 16, 32, 64):
                bsr, csr = res[("bsr", k)], res[("csr", k)]
                print(json.dumps({"case": f"{name}_b{b}", "n": n, "b": b, "k": k, "nnzb": int(indptr[-1]),
                                  "entries_per_row": round(float(indptr[-1]) * b / n, 1), "bsr": bsr, "csr": csr,
                                  "speedup_kernel": round(csr["kernel_ms"] / bsr["kernel_ms"], 2),
                                  "setup_s": {"bsr": round(setup_bsr, 2), "csr": round(setup_csr, 2), "build": round(build_s, 2)}}),
                      flush=True)
            del indptr, bj, vals


if __name__ == "__main__":
    main()
