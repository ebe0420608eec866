"""Checker tool (not collected by pytest): new values on the kept pattern of a sparse operator at N = 10^6 - dav_update_operator_values_dev
(fortran_davidson_amd/csrc/k_sparse_refresh.hip, k_bsr_build.hip) against the set entries it replaces in a loop, in the same process: the
three CSR classes of csr_setup_sweep.py and the block band of bsr_setup_sweep.py with b = 4, 8, 16, given in full (FULL) and as the lower
triangle (LOWER), entries in column order.  Per case: the host set entry (once), the device set entry (median of --reps), the device set
entry with dav_keep_value_map on (once), the device update (median of --reps) and the host update (once); all calls return synchronised,
so a host clock measures them, and a warm-up of each entry comes first.  Every case checks the updated operator bitwise (diagonal and
one 16-column apply) against a FRESH device set call with the new values, and reads the cost of the map from dav_device_memory around
the set call of a fresh engine with and without it (model: 8 bytes per canonical entry or block, 16 per row or block row).  The first
line gives the read rate of the box (dav_bench_stream3); every case carries the byte model of the value kernel (24 bytes per canonical
entry, 16 b^2 + 8 per canonical block) - kernel times come from a separate run under a kernel trace.  One JSON line per case on stdout.
    python tests/sparse_refresh_sweep.py [--n 1000000] [--reps 3] [--cases banded65,uniform64,skewed64,band4,band8,band16]
                                         [--triangles FULL,LOWER]
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
from fortran_davidson_amd.engine_c import BSR_ROW_MAJOR, OP_A, PANEL_V, PANEL_W  # noqa: E402
from bsr_apply_sweep import block_band                                   # noqa: E402
from csr_setup_sweep import reorder                                      # noqa: E402
from sparse_apply_sweep import banded, skewed, uniform                   # noqa: E402

DEV = "cuda:0"


def new_values(vv):
    return np.where(np.abs(vv) < 0.5, 1.25 * vv, vv + 3.0 + 0.1 * np.abs(vv))


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="banded65,uniform64,skewed64,band4,band8,band16")
    ap.add_argument("--triangles", default="FULL,LOWER")
    args = ap.parse_args()
    n = args.n
    rng = np.random.default_rng(2026)
    x = rng.standard_normal((n, 16))
    csr = {"banded65": lambda: banded(n), "uniform64": lambda: uniform(n, rng), "skewed64": lambda: skewed(n, rng)}
    warm = set()
    with fd.CEngine(n=n, max_cols=16) as e:
        def apply():
            e.panel_put(PANEL_V, 0, x)
            e.apply(OP_A, PANEL_V, 0, 16, PANEL_W, 0)
            return e.panel_get(PANEL_W, 0, 16)

        _, _, read_gbps = e.bench_stream3(0, 5)
        print(json.dumps({"case": "stream", "read_GBps": round(read_gbps, 1)}), flush=True)
        for case in args.cases.split(","):
            b = int(case[4:]) if case.startswith("band") and case[4:].isdigit() else 0
            if b:
                indptr, bj, vals = block_band(n, b)
                nrows = n // b
                rows = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(indptr))
                cols = bj
            else:
                indptr, cols, vals = csr[case]()
                nrows = n
                cols, vals, rows = reorder(indptr, cols, vals, rng, False)
            for tri in args.triangles.split(","):
                lower = tri == "LOWER"
                if lower:
                    keep = cols <= rows
                    rp = np.zeros(nrows + 1, dtype=np.int64)
                    np.cumsum(np.bincount(rows[keep], minlength=nrows), out=rp[1:])
                    cc, vv = np.ascontiguousarray(cols[keep]), np.ascontiguousarray(vals[keep])
                    canonical = int(2 * cc.size - np.count_nonzero(cc == rows[keep]))
                else:
                    rp, cc, vv, canonical = indptr, cols, vals, int(cols.size)
                vv2 = new_values(vv)
                d_ix = (torch.from_numpy(rp).to(DEV), torch.from_numpy(np.ascontiguousarray(cc)).to(DEV))
                d_old, d_new = torch.from_numpy(vv).to(DEV), torch.from_numpy(vv2).to(DEV)
                torch.cuda.synchronize()
                if b:
                    set_host = lambda eng, v: eng.set_operator_bsr(OP_A, rp, cc, v, lower=lower, layout=BSR_ROW_MAJOR)          # noqa: E731
                    set_dev = lambda eng, v: eng.set_operator_bsr_dev(OP_A, *d_ix, v, lower=lower, layout=BSR_ROW_MAJOR)        # noqa: E731
                else:
                    set_host = lambda eng, v: eng.set_operator_csr(OP_A, rp, cc, v, lower=lower)                                # noqa: E731
                    set_dev = lambda eng, v: eng.set_operator_csr_dev(OP_A, *d_ix, v, lower=lower)                              # noqa: E731
                kind = "bsr" if b else "csr"
                if kind not in warm:                       # every entry once before anything is timed
                    e.keep_value_map(OP_A, True)
                    set_host(e, vv)
                    set_dev(e, d_old)
                    e.update_operator_values(OP_A, d_new)
                    e.update_operator_values(OP_A, vv2)
                    warm.add(kind)
                e.keep_value_map(OP_A, False)
                host_s = timed(lambda: set_host(e, vv))
                dev_all = [timed(lambda: set_dev(e, d_new)) for _ in range(args.reps)]
                d_ref, y_ref = e.get_diagonal(OP_A), apply()              # the yardstick: a fresh set call with the new values
                e.keep_value_map(OP_A, True)
                dev_map_s = timed(lambda: set_dev(e, d_old))
                upd_all = []
                for r in range(2 * args.reps):                            # old and new values in turn; the last update brings the new ones
                    t = timed(lambda: e.update_operator_values(OP_A, d_new if r % 2 else d_old))
                    if r % 2:
                        upd_all.append(t)
                d_upd, y_upd = e.get_diagonal(OP_A), apply()
                same = bool(np.array_equal(d_ref.view(np.uint64), d_upd.view(np.uint64)) and
                            np.array_equal(y_ref.view(np.uint64), y_upd.view(np.uint64)))
                e.update_operator_values(OP_A, vv)
                upd_host_s = timed(lambda: e.update_operator_values(OP_A, vv2))
                same = same and bool(np.array_equal(d_ref.view(np.uint64), e.get_diagonal(OP_A).view(np.uint64)) and
                                     np.array_equal(y_ref.view(np.uint64), apply().view(np.uint64)))
                used = []
                for on in (False, True):                                  # the cost of the map: a fresh engine with and without it
                    with fd.CEngine(n=n, max_cols=16) as m:
                        fd.free_buffers()
                        m.keep_value_map(OP_A, on)
                        before = m.device_memory()[0]
                        set_dev(m, d_old)
                        used.append(before - m.device_memory()[0])
                dev_s, upd_s = float(np.median(dev_all)), float(np.median(upd_all))
                print(json.dumps({"case": case, "triangle": tri, "n": n, "given": int(cc.size), "canonical": canonical,
                                  "value_model_bytes": canonical * (16 * b * b + 8 if b else 24),
                                  "host_set_ms": round(1e3 * host_s, 1), "device_set_ms": round(1e3 * dev_s, 2),
                                  "device_set_ms_all": [round(1e3 * t, 2) for t in dev_all],
                                  "device_set_with_map_ms": round(1e3 * dev_map_s, 2), "device_update_ms": round(1e3 * upd_s, 3),
                                  "device_update_ms_all": [round(1e3 * t, 3) for t in upd_all],
                                  "host_update_ms": round(1e3 * upd_host_s, 1), "set_over_update": round(dev_s / upd_s, 1),
                                  "map_bytes_measured": used[1] - used[0], "map_bytes_model": 8 * canonical + 16 * nrows + 8,
                                  "bitwise_equal": same}), flush=True)
                del d_ix, d_old, d_new
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
