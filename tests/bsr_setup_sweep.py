"""Checker tool (not collected by pytest): set-up time of a BSR operator at N = 10^6 - the host entry dav_set_operator_bsr against the
device entry dav_set_operator_bsr_dev (fortran_davidson_amd/csrc/k_csr_build.hip, k_bsr_build.hip) in the same process, for b = 4, 8, 16
on the two patterns of bsr_apply_sweep.py (block band, uniformly random block columns), given in full (FULL) and as the lower block
triangle (LOWER), with row- and column-major blocks, the blocks of every block row in column order and shuffled.  Both calls return
synchronised, so a host clock measures them.  A warm-up call of each entry comes first; the device entry is timed as the median of
--reps calls.  Every case also checks that the two builds agree (diagonal and one 16-column apply, bitwise).  The first line gives the
read rate of the box (dav_bench_stream3); every case carries the byte model of the gather / transpose kernel (16 b^2 + 12 bytes per
canonical block) - its time comes from a separate run under a kernel trace, narrowed with the filters below so that every gather of
the run is of one kind (FULL row-major: all blocks transposed; FULL column-major: all copied).  One JSON line per case on stdout.
    python tests/bsr_setup_sweep.py [--n 1000000] [--reps 3] [--bs 4,8,16] [--patterns band,uniform] [--triangles FULL,LOWER]
                                    [--layouts row,col] [--orders sorted,shuffled]
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
import fortran_davidson_amd as fd                                                          # noqa: E402
from fortran_davidson_amd.engine_c import BSR_COL_MAJOR, BSR_ROW_MAJOR, OP_A, PANEL_V, PANEL_W  # noqa: E402
from bsr_apply_sweep import block_band, block_uniform                                      # noqa: E402


def reorder(indptr, bj, rng, shuffle):
    """permutation that puts the blocks of every block row in column order, or in a random order"""
    nb = indptr.size - 1
    bi = np.repeat(np.arange(nb, dtype=np.int64), np.diff(indptr))
    sub = rng.integers(0, 2**31, bi.size) if shuffle else bj.astype(np.int64)
    return np.argsort(bi * 2**31 + sub, kind="stable"), bi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bs", default="4,8,16")
    ap.add_argument("--patterns", default="band,uniform")
    ap.add_argument("--triangles", default="FULL,LOWER")
    ap.add_argument("--layouts", default="row,col")
    ap.add_argument("--orders", default="sorted,shuffled")
    args = ap.parse_args()
    n = args.n
    rng = np.random.default_rng(2026)
    x = rng.standard_normal((n, 16))
    with fd.CEngine(n=n, max_cols=16) as e:
        def apply():
            e.panel_put(PANEL_V, 0, x)
            e.apply(OP_A, PANEL_V, 0, 16, PANEL_W, 0)
            return e.panel_get(PANEL_W, 0, 16)

        _, _, read_gbps = e.bench_stream3(0, 5)
        print(json.dumps({"case": "stream", "read_GBps": round(read_gbps, 1)}), flush=True)
        warm = True
        for b in [int(s) for s in args.bs.split(",")]:
            for pattern in args.patterns.split(","):
                indptr, bj, vals = block_band(n, b) if pattern == "band" else block_uniform(n, b, rng)
                nb = n // b
                for order in args.orders.split(","):
                    perm, bi = reorder(indptr, bj, rng, order == "shuffled")
                    for tri in args.triangles.split(","):
                        lower = tri == "LOWER"
                        sel = perm[bj[perm] <= bi[perm]] if lower else perm
                        rp = np.zeros(nb + 1, dtype=np.int64)
                        np.cumsum(np.bincount(bi[sel], minlength=nb), out=rp[1:])
                        cc = np.ascontiguousarray(bj[sel])
                        canonical = int(2 * cc.size - np.count_nonzero(cc == bi[sel])) if lower else int(cc.size)
                        for layout in args.layouts.split(","):
                            vv = np.ascontiguousarray(vals[sel] if layout == "row" else vals[sel].transpose(0, 2, 1))
                            lay = BSR_ROW_MAJOR if layout == "row" else BSR_COL_MAJOR
                            dev = (torch.from_numpy(rp).to("cuda:0"), torch.from_numpy(cc).to("cuda:0"), torch.from_numpy(vv).to("cuda:0"))
                            torch.cuda.synchronize()
                            if warm:
                                e.set_operator_bsr(OP_A, rp, cc, vv, lower=lower, layout=lay)
                                e.set_operator_bsr_dev(OP_A, *dev, lower=lower, layout=lay)
                                warm = False
                            t0 = time.perf_counter()
                            e.set_operator_bsr(OP_A, rp, cc, vv, lower=lower, layout=lay)
                            host_s = time.perf_counter() - t0
                            d_host, y_host = e.get_diagonal(OP_A), apply()
                            times = []
                            for _ in range(args.reps):
                                t0 = time.perf_counter()
                                e.set_operator_bsr_dev(OP_A, *dev, lower=lower, layout=lay)
                                times.append(time.perf_counter() - t0)
                            d_dev, y_dev = e.get_diagonal(OP_A), apply()
                            same = bool(np.array_equal(d_host.view(np.uint64), d_dev.view(np.uint64)) and
                                        np.array_equal(y_host.view(np.uint64), y_dev.view(np.uint64)))
                            dev_s = float(np.median(times))
                            print(json.dumps({"pattern": pattern, "b": b, "blocks": order, "triangle": tri, "layout": layout, "n": n,
                                              "nnzb_given": int(cc.size), "nnzb_canonical": canonical,
                                              "gather_model_bytes": canonical * (16 * b * b + 12),
                                              "host_ms": round(1e3 * host_s, 1), "device_ms": round(1e3 * dev_s, 2),
                                              "device_ms_all": [round(1e3 * t, 2) for t in times], "speedup": round(host_s / dev_s, 1),
                                              "bitwise_equal": same}), flush=True)
                            del dev, vv
                            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
