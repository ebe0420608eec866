"""Checker tool (not collected by pytest): scalar DPR against the Chebyshev-filtered correction (method "CHEB") at N = 10^6, with the
filter step inside the CSR product (the default) and as a launch of its own (DAV_CHEB_FUSE=0; the knob is read when an engine is
created, so each setting gets engines of its own).  Two matrices: the banded one of tests/sparse_apply_sweep.py (65 stored entries per
row, diagonal 1 .. N: the case made for DPR) and the 7-point Laplacian of a 100^3 grid with a perturbed diagonal, lowest 8 (a nearly
constant diagonal: the case made for the filter).  Per matrix, setting and method: iterations, block applies and column sweeps of A, the
wall time of `--reps` cold solves after one warm-up solve (median, minimum, maximum; the solves return synchronised, so a host clock
measures them).  Then the time of one filter step per column: Ritz phases of 8 columns at degrees 1 and 21 on a CEngine differ by 20
steps; median of `--reps`, against the byte model 12 nnz + 8 (N + 1) + (32 fused | 48 separate) N bytes per column at the read rate of
the box (dav_bench_stream3); and what the first correction on an operator costs more than a later one (the row-sum bound and the
workspace).  One JSON line per measurement on stdout.  `--root DIR --methods DPR --fuse 1 --no-step` runs the DPR solves alone on the
package of another checkout (the parent commit, for the comparison on the same box).
    python tests/cheb_sweep.py [--n 1000000] [--reps 5] [--tol 1e-8] [--max-iterations 400] [--cases banded,laplacian]
                               [--methods DPR,CHEB] [--fuse 1,0] [--no-step] [--root DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fortran_davidson_amd as fd                                        # noqa: E402
from fortran_davidson_amd.engine_c import OP_A, PANEL_V, PANEL_W          # noqa: E402
from sparse_apply_sweep import banded                                     # noqa: E402


def laplacian3d(nx, sigma=0.05, seed=1):
    """(indptr, indices, data) of the 7-point Laplacian of an nx^3 grid (Dirichlet) with the diagonal 6 + sigma N(0, 1)"""
    n = nx ** 3
    idx = np.arange(n, dtype=np.int64)
    i, j, k = idx // (nx * nx), (idx // nx) % nx, idx % nx
    cols = [idx]
    vals = [6.0 + sigma * np.random.default_rng(seed).standard_normal(n)]
    keep = [np.ones(n, dtype=bool)]
    for coord, step in ((i, nx * nx), (j, nx), (k, 1)):
        for sign in (-1, 1):
            keep.append((coord + sign >= 0) & (coord + sign < nx))
            cols.append(idx + sign * step)
            vals.append(np.full(n, -1.0))
    keep, cols, vals = np.stack(keep, 1), np.stack(cols, 1), np.stack(vals, 1)
    order = np.argsort(np.where(keep, cols, n), axis=1, kind="stable")
    keep, cols, vals = (np.take_along_axis(x, order, 1) for x in (keep, cols, vals))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(keep.sum(1), out=indptr[1:])
    return indptr, cols[keep].astype(np.int32), vals[keep]


def spread(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(float(min(xs)), 3), "max": round(float(max(xs)), 3)}


def solves(name, arrays, n, lowest, fuse, args):
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_sparse(1, *arrays)
        for method in [m for m in args.methods.split(",") if fuse == "1" or m != "DPR"]:
            times, iters, st = [], None, None
            for rep in range(args.reps + 1):
                eng.c.reset_stats()
                t0 = time.perf_counter()
                _, _, iters = eng.solve(method, args.max_iterations, args.tol, want_vectors=False)
                if rep > 0:
                    times.append(1e3 * (time.perf_counter() - t0))
                st = eng.c.stats()
            print(json.dumps({"case": name, "n": n, "lowest": lowest, "method": method, "fused_step": fuse == "1", "iters": iters,
                              "converged": iters <= args.max_iterations, "applies": st.applies, "column_sweeps": st.apply_cols,
                              "wall_ms": spread(times)}), flush=True)


def step_time(name, arrays, n, fuse, read_gbps, args, k=8):
    from fortran_davidson_amd.engine_c import method_cheb
    nnz = int(arrays[0][-1])
    rng = np.random.default_rng(3)
    v = np.linalg.qr(rng.standard_normal((n, k)))[0]
    with fd.CEngine(n=n, max_cols=2 * k) as e:
        e.set_operator_csr(OP_A, *arrays)
        e.panel_put(PANEL_V, 0, v)
        e.apply(OP_A, PANEL_V, 0, k, PANEL_W, 0)
        w = e.panel_get(PANEL_W, 0, k)
        theta, y = np.linalg.eigh(v.T @ w)
        y = np.asfortranarray(y)
        ms, first = {}, None
        for degree in (1, 21):
            ts = []
            for rep in range(args.reps + 1):
                e.panel_put(PANEL_V, 0, v)
                e.synchronize()
                t0 = time.perf_counter()
                e.ritz_residual_correction(k, k, y, theta, method_cheb(degree))
                if rep > 0:
                    ts.append(1e3 * (time.perf_counter() - t0))
                elif degree == 1:
                    first = 1e3 * (time.perf_counter() - t0)
            ms[degree] = ts
    per_step = [(b - a) / 20.0 for a, b in zip(sorted(ms[1]), sorted(ms[21]))]
    model = 12.0 * nnz + 8.0 * (n + 1) + (32.0 if fuse == "1" else 48.0) * n * k
    med = float(np.median(per_step))
    print(json.dumps({"case": name, "n": n, "columns": k, "fused_step": fuse == "1", "step_ms": spread(per_step),
                      "step_us_per_column": round(1e3 * med / k, 2), "model_bytes": model, "GBps": round(model / (med * 1e6), 1),
                      "fraction_of_read_rate": round(model / (med * 1e6) / read_gbps, 3),
                      "first_correction_extra_ms": round(first - float(np.median(ms[1])), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iterations", type=int, default=400)
    ap.add_argument("--cases", default="banded,laplacian")
    ap.add_argument("--methods", default="DPR,CHEB")
    ap.add_argument("--fuse", default="1,0")
    ap.add_argument("--no-step", action="store_true", help="skip the time of one filter step")
    ap.add_argument("--root", default=None, help="the checkout whose package is measured (default: this one)")
    args = ap.parse_args()
    nx = round(args.n ** (1.0 / 3.0))
    cases = {"banded": lambda: (banded(args.n), args.n, 16), "laplacian": lambda: (laplacian3d(nx), nx ** 3, 8)}
    with fd.CEngine(n=args.n, max_cols=16) as e:
        _, _, read_gbps = e.bench_stream3(0, 5)
    print(json.dumps({"case": "stream", "read_GBps": round(read_gbps, 1)}), flush=True)
    for name in args.cases.split(","):
        arrays, n, lowest = cases[name]()
        for fuse in args.fuse.split(","):
            os.environ["DAV_CHEB_FUSE"] = fuse
            solves(name, arrays, n, lowest, fuse, args)
            if not args.no_step:
                step_time(name, arrays, n, fuse, read_gbps, args)


if __name__ == "__main__":
    main()
