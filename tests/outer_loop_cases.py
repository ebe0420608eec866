"""Shared by the recorder and the replay of the outer loop's footprints (tests/record_outer_loop.py, tests/test_outer_loop_gpu.py; not
collected): one small solve per branch of the driver loops in fortran/davidson_loop.f90 - growth, collapse restart, refresh, the three
correction entries, device Rayleigh-Ritz, the probe of the wanted pairs, the three policies, warm start, host callbacks, the one-shot
front ends, three ranks.  A footprint is what a solve leaves behind that does not depend on rounding: `iters`, and for a resident
DavidsonEngine the engine's counters after reset_stats(); the eigenvalues go with it.

The fixture tests/golden/outer_loop_footprints.json is recorded from the PARENT of the commit that restructures the loop (its package
first on the path), never from the code under test: tests/record_outer_loop.py."""
import ctypes as C
import threading

import numpy as np

from oracle import davidson_oracle as O
import cheb_inputs as CI

COUNTERS = ("applies", "apply_cols", "apply_launches", "restarts", "collectives", "m")
TOL = 1e-8


def matrices(n, sp, seed, gev=False, clustered=0):
    """generated diagonally dominant A (seed) and SPD B (seed + 100), as tests/test_solver_gpu.py and tests/test_policy_gpu.py build
    them; clustered = L > 0: the first L diagonal entries of tests/test_policy_gpu.py, whose pairs converge at different iterations"""
    a = O.generate_diagonal_dominant(n, sp, seed=seed)
    b = O.generate_diagonal_dominant(n, sp, 1.0, seed=seed + 100) if gev else None
    if clustered:
        d = np.arange(1, n + 1, dtype=float) + 2.0
        d[:clustered] = np.cumsum([1.0] + [0.08 if i % 2 else 1.7 for i in range(clustered - 1)])
        a[np.arange(n), np.arange(n)] = d
    return a, b


def case(kind="engine", n=300, lowest=4, sp=1e-2, seed=1, gev=False, clustered=0, method="DPR", policy="all", max_dim=None, drr=False,
         max_it=200, tol=TOL, env=None, check=None, counters=True, nranks=1, guess=None):
    return dict(kind=kind, n=n, lowest=lowest, sp=sp, seed=seed, gev=gev, clustered=clustered, method=method, policy=policy,
                max_dim=max_dim, drr=drr, max_it=max_it, tol=tol, env=env or {}, check=check, counters=counters, nranks=nranks, guess=guess)


REFRESH_1, REFRESH_2 = {"DAV_REFRESH_EVERY": "1"}, {"DAV_REFRESH_EVERY": "2"}
# name -> case; `check`: the condition the recorder asserts on the parent's footprint (f: the footprint) before it writes the fixture,
# so that a case cannot silently miss its branch
CASES = {
    # 1-3: the reference's policy - growth only; collapse restarts; every second restart re-applies the operators
    "all_dpr_std": case(check=lambda f: f["restarts"] == 0),
    "all_dpr_std_restarts": case(max_dim=8, check=lambda f: f["restarts"] >= 1),
    "all_dpr_std_refresh2": case(max_dim=8, env=REFRESH_2, check=lambda f: f["restarts"] >= 4),
    # 4-5: GJD (dav_gjd_correction_n for all pairs), generalized restarts (restart_transform)
    "all_gjd_std": case(n=200, lowest=3, sp=5e-2, seed=5, method="GJD", max_it=60),
    "all_gjd_gev_restarts": case(n=200, lowest=3, sp=5e-2, seed=5, gev=True, method="GJD", max_dim=10, max_it=60,
                                 check=lambda f: f["restarts"] >= 1),
    "all_dpr_gev_restarts": case(n=200, lowest=3, sp=5e-2, seed=5, gev=True, max_dim=10, check=lambda f: f["restarts"] >= 1),
    # 6: Rayleigh-Ritz on the device - dav_rr_restart, dav_rr_get before a generalized restart, GJD
    "drr_dpr_std_restarts": case(max_dim=8, drr=True, check=lambda f: f["restarts"] >= 1),
    "drr_dpr_gev_restarts": case(n=200, lowest=3, sp=5e-2, seed=5, gev=True, max_dim=10, drr=True, check=lambda f: f["restarts"] >= 1),
    "drr_gjd_std": case(n=200, lowest=3, sp=5e-2, seed=5, method="GJD", drr=True, max_it=60),
    # 7: a method that is neither DPR nor GJD on a CSR Laplacian (cheb_inputs) - the _n entry of the Ritz phase on the host, the
    # prefetched Gram blocks of a block made in the Ritz phase on the device
    "cheb_csr": case(kind="cheb", lowest=4, method="CHEB", max_it=60),
    "cheb_csr_drr": case(kind="cheb", lowest=4, method="CHEB", drr=True, max_it=60),
    # 8: policy "unconverged"; max_dim_sub < 2 * lowest leaves cap = m = 2 * lowest: the growth rule's `m < cap` stops every iteration at a
    # restart, so the basis never grows (the cap - m clamp of the correction count cannot bind here or anywhere: an iteration that grows has
    # m + lowest <= max_dim < cap, or m = 2 * lowest with cap >= 4 * lowest)
    "unconverged_dpr_std": case(n=200, lowest=3, sp=5e-2, seed=5, policy="unconverged", max_dim=10, check=lambda f: f["restarts"] >= 1),
    "unconverged_gjd_gev": case(n=200, lowest=3, sp=5e-2, seed=5, gev=True, method="GJD", policy="unconverged", max_dim=10, max_it=60),
    "unconverged_dpr_drr": case(n=200, lowest=3, sp=5e-2, seed=5, policy="unconverged", max_dim=10, drr=True),
    "unconverged_narrow_cap": case(policy="unconverged", max_dim=6, max_it=5, check=lambda f: f["iters"] == 6),
    # 9-10: policy "locking" - standard with restarts, GJD, generalized (guard vectors); the same with a refresh at every contraction
    "locking_dpr_std_restarts": case(n=400, lowest=8, sp=3e-2, seed=4, clustered=8, policy="locking", max_dim=28, max_it=300,
                                     check=lambda f: f["restarts"] >= 1),
    "locking_gjd_std": case(n=200, lowest=3, sp=1e-2, seed=3, method="GJD", policy="locking", max_it=100),
    "locking_dpr_gev": case(n=400, lowest=8, sp=5e-2, seed=3, gev=True, clustered=8, policy="locking", max_dim=24),
    "locking_dpr_std_refresh1": case(n=400, lowest=8, sp=3e-2, seed=4, clustered=8, policy="locking", max_dim=28, max_it=300, env=REFRESH_1),
    "locking_dpr_gev_refresh1": case(n=400, lowest=8, sp=5e-2, seed=3, gev=True, clustered=8, policy="locking", max_dim=24, env=REFRESH_1),
    # 11: the probe of the wanted pairs at m >= 48.  Whether it ran does not show in the counters; confirmed when the fixture was
    # recorded, with DAVIDSON_VERBOSE=2: lowest = 8 enters iteration 7 at m = 64 with residuals below sqrt(tolerance) and converges in the
    # probe (a subset solve, 8 * 8 = 64: that iteration prints no trace line); lowest = 12 enters iteration 5 at m = 48 with residuals
    # below 1e-4 (8 * 12 > 48: have_all_pairs, the full problem is not solved again), then converges at m = 96
    "probe_subset": case(n=400, lowest=8, seed=7, tol=1e-12, check=lambda f: f["m"] >= 48 and f["iters"] >= 2),
    "probe_all_pairs": case(n=400, lowest=12, sp=5e-2, seed=7, max_dim=50, check=lambda f: f["m"] >= 48 and f["iters"] >= 2),
    # 12: fewer columns left in the space than corrections (kt = min(., n - m))
    "tiny_all": case(n=20, lowest=4, seed=2, max_it=50, check=lambda f: f["m"] == 20),
    "tiny_unconverged": case(n=20, lowest=4, seed=2, policy="unconverged", max_it=50),
    # 13: out of iterations (the last Ritz pairs; the locking loop's non-converged exit)
    "max_it_all": case(max_dim=8, max_it=3, counters=False, check=lambda f: f["iters"] == 4),
    "max_it_locking": case(n=400, lowest=8, sp=3e-2, seed=4, clustered=8, policy="locking", max_dim=28, max_it=3, counters=False,
                           check=lambda f: f["iters"] == 4),
    # 14: warm start - two guess columns (unit vectors fill the start basis); a second solve from the first one's Ritz vectors
    "warm_two_columns": case(guess="columns"),
    "warm_previous_result": case(guess="previous"),
    # 15: the matrix-free front end with numpy callbacks; with restarts the callbacks are re-applied to the kept block
    "free_callbacks": case(kind="free", n=200, lowest=3, sp=5e-3, seed=41, gev=True, max_dim=30, counters=False),
    "free_callbacks_refresh1": case(kind="free", n=200, lowest=3, sp=5e-3, seed=41, gev=True, max_dim=6, env=REFRESH_1, counters=False),
    # 16: the one-shot front ends (the Python doors of the sparse ones take no preconditioner: M goes to slot 3 of an engine)
    "oneshot_dense": case(kind="dense", n=200, lowest=3, sp=5e-2, seed=5, gev=True, counters=False),
    "oneshot_sparse": case(kind="sparse", lowest=4, counters=False),
    "engine_sparse_preconditioner": case(kind="precond", lowest=4),
    # 17: three loopback ranks, as tests/test_policy_gpu.py runs them
    "ranks3_all_dpr_restarts": case(max_dim=8, nranks=3, check=lambda f: f["restarts"] >= 1),
    "ranks3_locking": case(n=400, lowest=8, sp=3e-2, seed=4, clustered=8, policy="locking", max_dim=28, max_it=300, nranks=3),
}


def _footprint(c, eng, out):
    lam, _, iters = out
    f = {"iters": int(iters), "eigenvalues": [float(x) for x in lam]}
    if c["counters"]:
        st = eng.c.stats()
        f.update({k: int(getattr(st, k)) for k in COUNTERS})
    return f


def _prepare(c, eng, a, b):
    if c["policy"] != "all":
        eng.set_correction_policy(c["policy"])
    if c["drr"]:
        eng.set_device_rr(True)
    if c["kind"] in ("cheb", "precond"):
        eng.set_sparse(1, *CI.csr_of(a))
        if c["kind"] == "precond":          # M = inv(A + I) as a full CSR matrix
            m = np.linalg.inv(a + np.eye(a.shape[0]))
            eng.set_sparse(3, *CI.csr_of(0.5 * (m + m.T)))
    else:
        eng.set_dense(1, a)
        if b is not None:
            eng.set_dense(2, b)


def run_case(c, fd):
    """the footprint of case c with the package fd (the environment of c["env"] is the caller's to set)"""
    from fortran_davidson_amd.solver import generalized_eigensolver_free, generalized_eigensolver_sparse
    n, L = c["n"], c["lowest"]
    if c["kind"] in ("cheb", "sparse", "precond"):
        a, b = CI.laplacian2d(16, 1), None
        n = a.shape[0]
    else:
        a, b = matrices(n, c["sp"], c["seed"], c["gev"], c["clustered"])
    if c["kind"] == "free":
        return _footprint(c, None, generalized_eigensolver_free(lambda x: a @ x, n, L, "DPR", c["max_it"], c["tol"], c["max_dim"],
                                                                lambda x: b @ x))
    if c["kind"] == "dense":
        return _footprint(c, None, fd.generalized_eigensolver(a, L, c["method"], c["max_it"], c["tol"], c["max_dim"], b))
    if c["kind"] == "sparse":
        return _footprint(c, None, generalized_eigensolver_sparse(*CI.csr_of(a), L, c["method"], c["max_it"], c["tol"], c["max_dim"]))
    nranks = c["nranks"]
    engs = [fd.DavidsonEngine(n, L, c["max_dim"], gev=c["gev"], rank=r, nranks=nranks) for r in range(nranks)]
    try:
        if nranks > 1:
            handles = (C.c_void_p * nranks)(*[e.c.h for e in engs])
            assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
        out, err = [None] * nranks, [None] * nranks

        def work(r):
            try:
                _prepare(c, engs[r], a, b)
                if c["guess"] == "previous":
                    engs[r].solve(c["method"], c["max_it"], 1e-4, reuse_vectors=True)
                engs[r].c.reset_stats()
                guess = np.linalg.qr(np.random.default_rng(3).standard_normal((n, 2)))[0] if c["guess"] == "columns" else None
                out[r] = engs[r].solve(c["method"], c["max_it"], c["tol"], initial_vectors=guess)
            except Exception as exc:      # noqa: BLE001
                err[r] = exc

        if nranks == 1:
            work(0)
        else:
            threads = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
            [t.start() for t in threads]
            [t.join(timeout=120) for t in threads]
        assert all(x is None for x in err), err
        assert all(o is not None for o in out), "a rank did not finish"
        assert all(o[2] == out[0][2] and np.array_equal(o[0], out[0][0]) for o in out)     # every rank holds the same answer
        return _footprint(c, engs[0], out[0])                  # (the counters are those of rank 0)
    finally:
        for e in engs:
            e.close()
