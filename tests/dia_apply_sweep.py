"""Checker tool (not collected by pytest): the block product of a CSR operator stored by diagonals (DAV_CSR_DIAGONALS,
fortran_davidson_amd/csrc/k_dia.hip) against the CSR product of the same matrix (k_spmm.hip) at N = 10^6, on one engine and in one run:
the matrix is set without and with the flag in turn (`--rounds` times), and after a warm-up of every shape each round times `--reps`
single applies at k = 8, 16 and 64 by device events (dav_bench_apply2 with one repetition: the kernel's own pair of events).  Matrices:
the 7-point Laplacian of a 100^3 grid (tests/cheb_sweep.py) and the banded matrix with 65 entries per row (tests/sparse_apply_sweep.py).
Per matrix, storage and k: median (minimum - maximum) of the kernel time, the byte model of the storage, GB/s and the fraction of the
read rate of the box (dav_bench_stream3); then whether the flagged apply is faster by more than the two spreads together.  Then one
"CHEB" solve of the Laplacian (lowest 8) and one "DPR" solve of the banded matrix (lowest 16) in both storages - one warm-up solve, three
cold solves, host clock around the synchronised call, median - and the set-call time and device memory of both storages.  One JSON line
per measurement on stdout.
    python tests/dia_apply_sweep.py [--n 1000000] [--reps 15] [--rounds 3] [--no-solves]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fortran_davidson_amd as fd                                        # noqa: E402
from fortran_davidson_amd.engine_c import OP_A                            # noqa: E402
from cheb_sweep import laplacian3d                                        # noqa: E402
from sparse_apply_sweep import banded                                     # noqa: E402

KS = (8, 16, 64)
STORAGES = (("csr", False), ("diagonals", True))


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def applies(name, arrays, n, read_gbps, args):
    times = {(s, k): [] for s, _ in STORAGES for k in KS}
    model, set_s, mem = {}, {s: [] for s, _ in STORAGES}, {}
    with fd.CEngine(n=n, max_cols=64) as e:
        for rnd in range(args.rounds + 1):                       # round 0 warms every shape up
            for s, flag in STORAGES:
                e.synchronize()
                t0 = time.perf_counter()
                e.set_operator_csr(OP_A, *arrays, diagonals=flag)
                e.synchronize()
                set_s[s].append(time.perf_counter() - t0)
                free, total = e.device_memory()
                mem[s] = round((total - free) / 2 ** 20, 1)
                for k in KS:
                    for _ in range(args.reps if rnd > 0 else 2):
                        _, kms, nbytes, _ = e.bench_apply2(k, 1)
                        if rnd > 0:
                            times[(s, k)].append(kms)
                    model[(s, k)] = nbytes
    for k in KS:
        row = {"case": name, "n": n, "k": k}
        for s, _ in STORAGES:
            sp = spread(times[(s, k)])
            gbps = model[(s, k)] / (sp["median"] * 1e-3) / 1e9
            row[s] = {"kernel_ms": sp, "model_bytes": model[(s, k)], "GBps": round(gbps, 1), "fraction_of_read_rate": round(gbps / read_gbps, 3)}
        c, d = row["csr"]["kernel_ms"], row["diagonals"]["kernel_ms"]
        row["speedup"] = round(c["median"] / d["median"], 2)
        row["faster_beyond_both_spreads"] = bool(c["median"] - d["median"] > (c["max"] - c["min"]) + (d["max"] - d["min"]))
        print(json.dumps(row), flush=True)
    nnz = int(arrays[0][-1])
    nd = int(np.unique(arrays[1].astype(np.int64) - np.repeat(np.arange(n, dtype=np.int64), np.diff(arrays[0]))).size)
    stored = {"csr": 12.0 * nnz + 8.0 * (n + 1), "diagonals": 8.0 * nd * ((n + 15) // 16 * 16) + 4.0 * nd}
    print(json.dumps({"case": name, "nnz": nnz, "nd": nd, "set_call_s": {s: spread(set_s[s][1:]) for s, _ in STORAGES},
                      "operator_MiB_model": {s: round(stored[s] / 2 ** 20, 1) for s, _ in STORAGES},
                      "device_MiB_in_use_after_set": mem}), flush=True)


def solves(name, arrays, n, lowest, method, args):
    row = {"case": "solve_" + name, "n": n, "lowest": lowest, "method": method}
    for s, flag in STORAGES:
        with fd.DavidsonEngine(n, lowest) as eng:
            eng.set_sparse(1, *arrays, diagonals=flag)
            ts, it = [], None
            for rep in range(4):
                eng.c.reset_stats()
                t0 = time.perf_counter()
                _, _, it = eng.solve(method, 400, 1e-8, want_vectors=False)
                if rep > 0:
                    ts.append(1e3 * (time.perf_counter() - t0))
            st = eng.c.stats()
        row[s] = {"iters": it, "applies": st.applies, "column_sweeps": st.apply_cols, "wall_ms": spread(ts), "apply_ms": round(st.apply_ms, 2)}
    row["speedup"] = round(row["csr"]["wall_ms"]["median"] / row["diagonals"]["wall_ms"]["median"], 2)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-solves", action="store_true")
    args = ap.parse_args()
    nx = round(args.n ** (1.0 / 3.0))
    with fd.CEngine(n=args.n, max_cols=16) as e:
        _, _, read_gbps = e.bench_stream3(0, 5)
    print(json.dumps({"case": "stream", "read_GBps": round(read_gbps, 1)}), flush=True)
    for name, make, lowest, method in (("laplacian7", lambda: (laplacian3d(nx), nx ** 3), 8, "CHEB"),
                                       ("banded65", lambda: (banded(args.n), args.n), 16, "DPR")):
        arrays, n = make()
        arrays = (arrays[0], arrays[1].astype(np.int32), arrays[2])
        applies(name, arrays, n, read_gbps, args)
        if not args.no_solves:
            solves(name, arrays, n, lowest, method, args)


if __name__ == "__main__":
    main()
