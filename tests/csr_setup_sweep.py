"""Checker tool (not collected by pytest): set-up time of a CSR operator at N = 10^6 - the host entry dav_set_operator_csr against the
device entry dav_set_operator_csr_dev (fortran_davidson_amd/csrc/k_csr_build.hip) in the same process, on the three matrix classes of
DESIGN section 12 (banded 65 per row, uniform 64 per row, skewed power law plus an arrowhead row), each with its rows in column order
and with the entries of every row shuffled, given in full (FULL) and as the lower triangle (LOWER).  Both calls return synchronised, so
a host clock measures them.  A warm-up call of each entry comes first; the device entry is timed as the median of --reps calls.  Every
case also checks that the two builds agree (diagonal and one 16-column apply, bitwise).  One JSON line per case on stdout.
    python tests/csr_setup_sweep.py [--n 1000000] [--reps 3]
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
import fortran_davidson_amd as fd                                # noqa: E402
from fortran_davidson_amd.engine_c import OP_A, PANEL_V, PANEL_W  # noqa: E402
from sparse_apply_sweep import banded, skewed, uniform            # noqa: E402


def reorder(indptr, cols, vals, rng, shuffle):
    """the entries of every row in column order, or in a random order"""
    n = indptr.size - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    sub = rng.integers(0, 2**31, rows.size) if shuffle else cols.astype(np.int64)
    order = np.argsort(rows * 2**31 + sub, kind="stable")
    return cols[order], vals[order], rows[order]


def lower_part(n, rows, cols, vals):
    keep = cols <= rows
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=indptr[1:])
    return indptr, cols[keep], vals[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    n = args.n
    rng = np.random.default_rng(2026)
    x = rng.standard_normal((n, 16))
    with fd.CEngine(n=n, max_cols=16) as e:
        def apply():
            e.panel_put(PANEL_V, 0, x)
            e.apply(OP_A, PANEL_V, 0, 16, PANEL_W, 0)
            return e.panel_get(PANEL_W, 0, 16)

        warm = True
        for cls, make in (("banded65", lambda: banded(n)), ("uniform64", lambda: uniform(n, rng)), ("skewed64", lambda: skewed(n, rng))):
            indptr, cols, vals = make()
            for shuffle in (False, True):
                c, v, r = reorder(indptr, cols, vals, rng, shuffle)
                for tri in ("FULL", "LOWER"):
                    rp, cc, vv = (indptr, c, v) if tri == "FULL" else lower_part(n, r, c, v)
                    lower = tri == "LOWER"
                    dev = (torch.from_numpy(rp).to("cuda:0"), torch.from_numpy(cc).to("cuda:0"), torch.from_numpy(vv).to("cuda:0"))
                    torch.cuda.synchronize()
                    if warm:
                        e.set_operator_csr(OP_A, rp, cc, vv, lower=lower)
                        e.set_operator_csr_dev(OP_A, *dev, lower=lower)
                        warm = False
                    t0 = time.perf_counter()
                    e.set_operator_csr(OP_A, rp, cc, vv, lower=lower)
                    host_s = time.perf_counter() - t0
                    d_host, y_host = e.get_diagonal(OP_A), apply()
                    times = []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        e.set_operator_csr_dev(OP_A, *dev, lower=lower)
                        times.append(time.perf_counter() - t0)
                    d_dev, y_dev = e.get_diagonal(OP_A), apply()
                    same = bool(np.array_equal(d_host.view(np.uint64), d_dev.view(np.uint64)) and
                                np.array_equal(y_host.view(np.uint64), y_dev.view(np.uint64)))
                    dev_s = float(np.median(times))
                    print(json.dumps({"class": cls, "rows": "shuffled" if shuffle else "sorted", "triangle": tri, "n": n,
                                      "nnz_given": int(rp[-1]), "host_ms": round(1e3 * host_s, 1), "device_ms": round(1e3 * dev_s, 2),
                                      "device_ms_all": [round(1e3 * t, 2) for t in times], "speedup": round(host_s / dev_s, 1),
                                      "bitwise_equal": same}), flush=True)
                    del dev
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
