"""GPU: CSR operators stored by diagonals (DAV_CSR_DIAGONALS; kernels in fortran_davidson_amd/csrc/k_dia.hip).  T1 exact products bit for
bit inside write fences; T2 the host and the device entry build the same storage; T3 real values within gamma(nd + 1), repeatable, and
independent of the block width; T4 three ranks equal one; T5 refusals; T6 new values on the kept pattern; T7 the Chebyshev correction,
fused and separate; T8 solves with and without the flag; T9 a Fortran program."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import (METHOD_DPR, OP_A, PANEL_R, PANEL_V, PANEL_W, DavidsonHipError, method_cheb)
import cheb_inputs as CI
import dia_inputs as D
from exact_inputs import (exact_sparse_product, fenced_apply, gamma, gram_is_exact, int_block, mismatch, run_ranks, same_bits,
                          unit_block)
from sparse_apply_sweep import banded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 5, 16, 17, 33, 48, 64, 66)          # 66: two launches
COLS = 96
C0, D0 = 3, 5                                # no multiples of 16
METHOD_BDPR = 3
FORMS = [(False, 0), (True, 0), (False, 1), (True, 1)]          # (lower, base)


def torch_arrays(rp, ci, vv, rp32=False):
    import torch
    return (torch.tensor(rp.astype(np.int32) if rp32 else rp, device="cuda"), torch.tensor(ci, device="cuda"), torch.tensor(vv, device="cuda"))


def set_dia(e, which, arrays, lower=False, base=0, entry="host", diagonals=True):
    if entry == "host":
        e.set_operator_csr(which, *arrays, base=base, lower=lower, diagonals=diagonals)
    else:
        e.set_operator_csr_dev(which, *torch_arrays(*arrays, rp32=base == 1), base=base, lower=lower, diagonals=diagonals)


def apply_fn(e, which=OP_A):
    return lambda sp, c0, k, dp, d0: e.apply(which, sp, c0, k, dp, d0)


def put_apply_get(e, x, which=OP_A):
    k = x.shape[1]
    e.panel_put(PANEL_V, 0, x)
    e.apply(which, PANEL_V, 0, k, PANEL_W, 0)
    return e.panel_get(PANEL_W, 0, k)


_pattern_cache = {}


def pattern_inputs(name):
    """(n, rows, cols, vals, X, Xs, A X, A Xs, a real X) of a T1 pattern, computed once"""
    if name not in _pattern_cache:
        n, r, c, v = D.pattern(name)
        rng = np.random.default_rng(len(name))
        x, xs = int_block(n, max(KS), rng), unit_block(n, max(KS), rng)
        _pattern_cache[name] = (n, r, c, v, x, xs, exact_sparse_product(n, r, c, v, x), exact_sparse_product(n, r, c, v, xs),
                                np.asfortranarray(rng.standard_normal((n, max(KS)))))
    return _pattern_cache[name]


# ---- T1: exact products, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.PATTERNS)
def test_exact_products_bit_for_bit_inside_write_fences(name):
    n, r, c, v, x, xs, ref, refs, _ = pattern_inputs(name)
    with fd.CEngine(n=n, max_cols=COLS) as e:
        for entry in ("host", "device"):
            for lower, base in FORMS:
                set_dia(e, OP_A, D.csr_form(n, r, c, v, lower, base), lower, base, entry)
                first = entry == "host" and (lower, base) == FORMS[0]
                for k in KS:
                    where = (name, entry, lower, base, k)
                    w, msgs = fenced_apply(e, x[:, :k], C0, D0, COLS, apply_fn(e), stale=k + 16 if first else 0)
                    ws, msgs2 = fenced_apply(e, xs[:, :k], C0, D0, COLS, apply_fn(e))
                    g = e.gram(PANEL_W, D0, k, PANEL_W, D0, k)
                    assert not msgs + msgs2, (where, msgs + msgs2)
                    assert same_bits(w, ref[:, :k]), (where, mismatch(w, ref[:, :k]))
                    assert same_bits(ws, refs[:, :k]), (where, mismatch(ws, refs[:, :k]))
                    assert gram_is_exact(g, ws), (where, "padding rows of the result are not zero")


# ---- T2: the same storage from both entries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.PATTERNS)
def test_host_and_device_entry_give_the_same_applies(name):
    n, r, c, v, *_, xr = pattern_inputs(name)
    vr = v * (1.0 + 0.25 * np.sin(3.0 * np.minimum(r, c) + 5.0 * np.maximum(r, c)))          # real values, still symmetric
    out = {}
    with fd.CEngine(n=n, max_cols=COLS) as e:
        for entry in ("host", "device"):
            for lower, base in FORMS:
                set_dia(e, OP_A, D.csr_form(n, r, c, vr, lower, base), lower, base, entry)
                out[(entry, lower, base)] = [put_apply_get(e, xr[:, :k]) for k in (5, 17, 64)]
    for lower, base in FORMS:
        for wh, wd in zip(out[("host", lower, base)], out[("device", lower, base)]):
            assert np.isfinite(wh).all() and wh.any()
            assert same_bits(wh, wd), (name, lower, base, mismatch(wh, wd))


# ---- T3: real values ------------------------------------------------------------------------------------------------------------------
def real_matrices():
    rp, ci, vv = banded(2000)
    return {"lap16": D.csr_of_dense(CI.laplacian2d(16)), "banded2000": (rp, ci.astype(np.int32), vv)}


@pytest.mark.parametrize("name", ["lap16", "banded2000"])
def test_real_values_within_gamma_repeatable_and_independent_of_the_width(name):
    rp, ci, vv = real_matrices()[name]
    n = rp.size - 1
    rows, cols, vals = D.canonical(n, rp, ci, vv)
    nd = D.offsets(rows, cols).size
    x = np.asfortranarray(np.random.default_rng(5).standard_normal((n, 64)) * np.exp(np.random.default_rng(6).uniform(-8, 8, (n, 1))))
    y_ld = np.zeros((n, 64), dtype=np.longdouble)
    np.add.at(y_ld, rows, vals.astype(np.longdouble)[:, None] * x.astype(np.longdouble)[cols])
    mag = np.zeros((n, 64))
    np.add.at(mag, rows, np.abs(vals)[:, None] * np.abs(x)[cols])
    with fd.CEngine(n=n, max_cols=64) as e:
        e.set_operator_csr(OP_A, rp, ci, vv, diagonals=True)
        e.reset_stats()
        w64 = put_apply_get(e, x)
        st = e.stats()
        assert st.apply_bytes == 8.0 * nd * n + 4.0 * nd + 16.0 * n * 64 and st.apply_flops == 2.0 * 64 * rows.size, (name, st.apply_bytes)
        again = put_apply_get(e, x)
        w16 = put_apply_get(e, x[:, :16])
        w1 = put_apply_get(e, x[:, 3:4])
    err = np.abs(w64.astype(np.longdouble) - y_ld).astype(np.float64)
    print(f"{name}: nd = {nd}, largest |Y - Y_ld| / (gamma(nd + 1) |A||X|) = {np.max(err / (gamma(nd + 1) * mag)):.3f}")
    assert (err <= gamma(nd + 1) * mag).all(), name
    assert same_bits(w64, again), name
    assert same_bits(w16, w64[:, :16]), (name, mismatch(w16, w64[:, :16]))
    assert same_bits(w1, w64[:, 3:4]), name


# ---- T4: three ranks equal one ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["band65", "stencil"])
def test_three_ranks_equal_one_bit_for_bit(name):
    n, r, c, v, *_, xr = pattern_inputs(name)
    dense = np.zeros((n, n))
    np.add.at(dense, (r, c), v / 64.0)
    dense[np.arange(n), np.arange(n)] = 10.0 + np.arange(n)          # a definite, well separated diagonal for the solve
    arrays = D.csr_of_dense(dense)
    lowest = 3

    def apply_of(e):
        e.set_operator_csr(OP_A, *arrays, diagonals=True)
        return [put_apply_get(e, xr[:, :k]) for k in (5, 33, 66)]

    with fd.CEngine(n=n, max_cols=COLS) as e:
        one = apply_of(e)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_sparse(1, *arrays, diagonals=True)
        lam1, _, it1 = eng.solve("DPR", 300, 1e-8, want_vectors=False)
    assert it1 < 300 and np.abs(lam1 - np.linalg.eigvalsh(dense)[:lowest]).max() < 1e-9
    outs = run_ranks(3, lambda rk: fd.CEngine(n=n, max_cols=COLS, rank=rk, nranks=3), lambda rk, e: (apply_of(e), e.local_rows()))
    for ws, (r0, nl) in outs:
        assert nl > 0
        for w3, w1 in zip(ws, one):
            assert same_bits(w3[r0:r0 + nl], w1[r0:r0 + nl]), (name, r0, mismatch(w3[r0:r0 + nl], w1[r0:r0 + nl]))

    def solve_of(rk, eng):
        eng.set_sparse(1, *arrays, diagonals=True)
        return eng.solve("DPR", 300, 1e-8, want_vectors=False)

    class Wrapped:                      # run_ranks joins and closes CEngine-like objects: the handle and close() of a DavidsonEngine
        def __init__(self, rk):
            self.eng = fd.DavidsonEngine(n, lowest, rank=rk, nranks=3)
            self.h = self.eng.c.h

        def close(self):
            self.eng.close()
    # the solve: the products are the same bits, the Gram sums of the Rayleigh-Ritz step are not - three ranks add their partial sums in
    # rank order, one rank has one sum - so the eigenvalues are compared as tests/test_sparse_gpu.py compares a three-rank CSR solve
    for lam3, _, it3 in run_ranks(3, Wrapped, lambda rk, wr: solve_of(rk, wr.eng)):
        print(f"{name}: three ranks against one, iterations {it3} / {it1}, largest eigenvalue difference {np.abs(lam3 - lam1).max():.3g}")
        assert it3 == it1 and np.abs(lam3 - lam1).max() < 1e-10, (name, it3, it1)


# ---- T5: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable():
    n = 301
    a = CI.random_sparse(n, 6 / n, 1)
    rp, ci, vv = D.csr_of_dense(a)
    rows, cols, _ = D.canonical(n, rp, ci, vv)
    nd = D.offsets(rows, cols).size
    good = D.csr_of_dense(CI.laplacian2d(16))
    x = np.asfortranarray(np.random.default_rng(1).standard_normal((n, 8)))
    lib = fd.hip_lib()
    with fd.CEngine(n=n, max_cols=16) as e:
        def usable():
            with pytest.raises(DavidsonHipError, match="operator not set"):
                e.apply(OP_A, PANEL_V, 0, 1, PANEL_W, 0)
            e.set_operator_csr(OP_A, rp, ci, vv)
            assert np.abs(put_apply_get(e, x) - a @ x).max() < 1e-12 * np.abs(a @ x).max()
        for entry in ("host", "device"):
            with pytest.raises(DavidsonHipError) as exc:
                set_dia(e, OP_A, (rp, ci, vv), entry=entry)
            msg = str(exc.value)
            assert f"nd = {nd}" in msg and f"{rows.size} entries" in msg and "DIA_MAX_FILL" in msg, msg
            usable()
        # a BSR entry with the flag, and flag words outside 0..3: straight to the C entries
        blocks = np.ones((n, 1, 1))
        rpb, cib = np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32)
        for tri in (2, 3):
            assert lib.dav_set_operator_bsr(e.h, OP_A, 1, rpb.ctypes.data, cib.ctypes.data, blocks.ctypes.data, 0, tri, 0) != 0
            msg = lib.dav_last_error().decode()
            assert "DAV_CSR_DIAGONALS" in msg and "CSR entries only" in msg, msg
            usable()
        for tri in (4, 7):
            for bsr in (False, True):
                if bsr:
                    rc = lib.dav_set_operator_bsr(e.h, OP_A, 1, rpb.ctypes.data, cib.ctypes.data, blocks.ctypes.data, 0, tri, 0)
                else:
                    rc = lib.dav_set_operator_csr(e.h, OP_A, rp.ctypes.data, ci.ctypes.data, vv.ctypes.data, 0, tri)
                assert rc != 0 and "triangle must be DAV_CSR_FULL or DAV_CSR_LOWER" in lib.dav_last_error().decode()
                usable()
    # BDPR on an operator stored by diagonals: refused with the panels untouched; an update without the map: refused
    n, m = 256, 5
    rng = np.random.default_rng(4)
    v, w = np.asfortranarray(rng.standard_normal((n, m))), np.asfortranarray(rng.standard_normal((n, m)))
    theta = np.sort(rng.uniform(-3.0, 3.0, m))
    with fd.CEngine(n=n, max_cols=16) as e:
        e.set_operator_csr(OP_A, *good, diagonals=True)
        mark = np.full((n, m), 3.25)
        e.panel_put(PANEL_V, m, mark)
        e.panel_put(PANEL_R, 0, mark)
        e.panel_put(PANEL_V, 0, v)
        e.panel_put(PANEL_W, 0, w)
        with pytest.raises(DavidsonHipError, match=re.escape("operator A is a CSR matrix stored by diagonals")) as exc:
            e.ritz_residual_correction(m, 1, np.eye(m), theta, METHOD_BDPR)
        assert "BDPR" in str(exc.value)
        assert same_bits(e.panel_get(PANEL_V, 0, m), v) and same_bits(e.panel_get(PANEL_W, 0, m), w)
        assert np.array_equal(e.panel_get(PANEL_V, m, m), mark) and np.array_equal(e.panel_get(PANEL_R, 0, m), mark)
        e.ritz_residual_correction(m, 1, np.eye(m), theta, METHOD_DPR)
        assert np.isfinite(e.panel_get(PANEL_V, m, m)).all()
        with pytest.raises(DavidsonHipError, match="set without its value map"):
            e.update_operator_values(OP_A, good[2])
        xx = np.asfortranarray(rng.standard_normal((n, 8)))
        ref = CI.laplacian2d(16) @ xx
        assert np.abs(put_apply_get(e, xx) - ref).max() < 1e-13 * np.abs(ref).max()


# ---- T6: new values on the kept pattern -----------------------------------------------------------------------------------------------------
def cheb_block(e, a, m=8, degree=6, seed=3):
    v = np.asfortranarray(np.linalg.qr(np.random.default_rng(seed).standard_normal((a.shape[0], m)))[0])
    w = np.asfortranarray(a @ v)
    theta, y = np.linalg.eigh(v.T @ w)
    e.panel_put(PANEL_V, 0, v)
    e.panel_put(PANEL_W, 0, w)
    e.ritz_residual_correction(m, 4, np.asfortranarray(y), theta, method_cheb(degree))
    return e.panel_get(PANEL_V, m, m)


@pytest.mark.parametrize("lower", [False, True])
def test_new_values_on_the_kept_pattern_equal_a_fresh_set_call(lower):
    import torch
    a1 = CI.laplacian2d(16, 1)
    a2 = np.where(a1 != 0.0, 1.75 * a1, 0.0) + np.diag(0.3 * np.cos(np.arange(256)))
    arr1, arr2 = D.csr_of_dense(a1, lower), D.csr_of_dense(a2, lower)
    assert np.array_equal(arr1[0], arr2[0]) and np.array_equal(arr1[1], arr2[1]) and CI.row_bound(a1) != CI.row_bound(a2)
    x = np.asfortranarray(np.random.default_rng(2).standard_normal((256, 33)))
    with fd.CEngine(n=256, max_cols=48) as e:
        e.set_operator_csr(OP_A, *arr2, lower=lower, diagonals=True)
        fresh, fresh_t, fresh_d = put_apply_get(e, x), cheb_block(e, a2), e.get_diagonal(OP_A)
    for source in ("host", "device"):
        with fd.CEngine(n=256, max_cols=48) as e:
            e.keep_value_map(OP_A)
            set_dia(e, OP_A, arr1, lower, 0, source)
            old, old_t = put_apply_get(e, x), cheb_block(e, a1)
            e.update_operator_values(OP_A, arr2[2] if source == "host" else torch.tensor(arr2[2], device="cuda"))
            new, new_t, new_d = put_apply_get(e, x), cheb_block(e, a2), e.get_diagonal(OP_A)
        assert not same_bits(old, new) and not same_bits(old_t, new_t)
        assert same_bits(new, fresh), (source, mismatch(new, fresh))
        assert same_bits(new_d, fresh_d)
        assert same_bits(new_t, fresh_t), (source, "the row bound did not follow the values")


# ---- T7: CHEB ---------------------------------------------------------------------------------------------------------------------------------
MS = (1, 5, 16, 17, 33)
DEGREES = (1, 2, 3, 10, 25)


def cheb_matrices():
    n, r, c, v = D.pattern("stencil")
    st = np.zeros((n, n))
    np.add.at(st, (r, c), v / 255.0)
    st[np.arange(n), np.arange(n)] = 6.0 + 0.05 * np.cos(np.arange(n))
    return {"lap16": CI.laplacian2d(16, 1), "stencil343": st}


def ritz_pairs(a, m, seed):
    v = np.linalg.qr(np.random.default_rng(seed).standard_normal((a.shape[0], m)))[0]
    w = a @ v
    theta, y = np.linalg.eigh(v.T @ w)
    return np.asfortranarray(v), np.asfortranarray(w), np.asfortranarray(y), theta


def correction(e, v, w, y, theta, lowest, method):
    m = v.shape[1]
    e.panel_put(PANEL_V, 0, v)
    e.panel_put(PANEL_W, 0, w)
    e.ritz_residual_correction(m, lowest, y, theta, method)
    return e.panel_get(PANEL_R, 0, m), e.panel_get(PANEL_V, m, m)


def check_block(a, prod, bound, r, t, theta, m, lowest, degree, where):
    """the check of tests/test_cheb_gpu.py: per column max |T - T_ld| <= 8 max(err_f64, d u) max |T_ld|"""
    t_ld = CI.cheb_correction(a, theta, r, m, lowest, degree, bound, np.longdouble, prod)
    t_64 = CI.cheb_correction(a, theta, r, m, lowest, degree, bound)
    scale = np.abs(t_ld).max(axis=0)
    assert (scale > 0).all(), where
    err64 = (np.abs(t_64 - t_ld).max(axis=0) / scale).astype(np.float64)
    err = (np.abs(t - t_ld).max(axis=0) / scale).astype(np.float64)
    bar = 8.0 * np.maximum(err64, degree * CI.U)
    ratio = float((err / bar).max())
    assert ratio <= 1.0, (where, ratio, err.max(), err64.max())
    return ratio


def cheb_blocks(e, a, ms=MS, degrees=DEGREES, check=True, key=""):
    prod, bound = CI.Product(a), CI.row_bound(a)
    out, worst = {}, 0.0
    for m in ms:
        v, w, y, theta = ritz_pairs(a, m, 1000 + m)
        lowest = min(4, m)
        for degree in degrees:
            r, t = correction(e, v, w, y, theta, lowest, method_cheb(degree))
            out[(m, degree)] = t
            if check:
                worst = max(worst, check_block(a, prod, bound, r, t, theta, m, lowest, degree, (key, m, degree)))
    return out, worst


@pytest.mark.parametrize("name", ["lap16", "stencil343"])
def test_cheb_block_matches_the_restatement_and_the_bound_is_the_csr_bound(name):
    a = cheb_matrices()[name]
    n = a.shape[0]
    with fd.CEngine(n=n, max_cols=66) as e:
        for lower in (False, True):
            e.set_operator_csr(OP_A, *D.csr_of_dense(a, lower), lower=lower, diagonals=True)
            _, worst = cheb_blocks(e, a, key=(name, lower))
            print(f"DIA {name} lower={lower}: largest error / bar = {worst:.3f}")
        # the bound, exactly: a correction of degree 1 is alpha_0 R with alpha_0 = 1 / (theta_0 - (a + b) / 2), b the bound and - with a
        # second Ritz value beyond it - a = b - (b - theta_0) / 64: a handful of float64 operations that the restatement repeats in the
        # same order.  Over three values of theta_0 either one-ulp neighbour of the bound changes the block
        bound = CI.row_bound(a)
        rng = np.random.default_rng(9)
        v, w = np.asfortranarray(rng.standard_normal((n, 2))), np.asfortranarray(rng.standard_normal((n, 2)))
        told = {nb: False for nb in (np.nextafter(bound, np.inf), np.nextafter(bound, -np.inf))}
        for theta0 in (0.0, -3.1, 0.777):
            theta = np.array([theta0, 2.0 * bound])
            r, t = correction(e, v, w, np.asfortranarray(np.eye(2)), theta, 1, method_cheb(1))
            assert same_bits(t, CI.cheb_correction(a, theta, r, 2, 1, 1, bound)), (name, theta0)
            for nb in told:
                told[nb] |= not same_bits(t, CI.cheb_correction(a, theta, r, 2, 1, 1, nb))
        assert all(told.values()), (name, told)


def test_fused_and_separate_step_agree_bit_for_bit(tmp_path):
    """DAV_CHEB_FUSE is read when an engine is created: the separate step runs in a fresh child process"""
    mats = cheb_matrices()
    ms = (1, 16, 17, 33)
    out = str(tmp_path / "separate.npz")
    env = dict(os.environ, DAV_CHEB_FUSE="0")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dia_cheb_child.py"), out], env=env, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    separate = np.load(out)
    for name, a in mats.items():
        with fd.CEngine(n=a.shape[0], max_cols=66) as e:
            e.set_operator_csr(OP_A, *D.csr_of_dense(a), diagonals=True)
            e.reset_stats()
            fused, _ = cheb_blocks(e, a, ms=ms, check=False)
            st = e.stats()
        for (m, degree), t in fused.items():
            assert np.isfinite(t).all() and t.any()
            assert same_bits(t, separate[f"{name}_{m}_{degree}"]), (name, m, degree)
        # that the knob was read: the same applies, and the fused ones account the bytes their epilogue reads
        assert (st.applies, st.apply_cols) == (int(separate[f"{name}_applies"]), int(separate[f"{name}_cols"]))
        extra = 8.0 * a.shape[0] * sum(ms) * sum(2 + 3 * (d - 2) for d in DEGREES if d >= 2)
        assert st.apply_bytes - float(separate[f"{name}_bytes"]) == extra, name


# ---- T8: solves -----------------------------------------------------------------------------------------------------------------------------
def banded_dense(n=2000):
    rp, ci, vv = banded(n)
    a = np.zeros((n, n))
    a[np.repeat(np.arange(n), np.diff(rp)), ci] = vv
    return a, (rp, ci.astype(np.int32), vv)


def check_pairs(a, b, lam, vec, ref, tol=1e-8):
    bx = vec if b is None else b @ vec
    assert np.linalg.norm(a @ vec - bx * lam[None, :], axis=0).max() < tol
    assert np.abs(lam - ref).max() < 1e-9


SOLVES = [("lap16", m, 4) for m in ("DPR", "GJD", "CHEB", "CHEB16")] + [("lap24", m, 8) for m in ("DPR", "GJD", "CHEB", "CHEB16")] + \
         [("banded2000", "DPR", 4)]
_solve_cache = {}


def solve_matrix(name):
    if name not in _solve_cache:
        if name == "banded2000":
            a, arrays = banded_dense()
        else:
            a = CI.laplacian2d(16, 1) if name == "lap16" else CI.laplacian2d(24, 2)
            arrays = D.csr_of_dense(a)
        _solve_cache[name] = (a, arrays, np.linalg.eigvalsh(a))
    return _solve_cache[name]


@pytest.mark.parametrize("name,method,lowest", SOLVES)
def test_solves_with_and_without_the_flag(name, method, lowest):
    a, arrays, ev = solve_matrix(name)
    its = {}
    for diagonals in (False, True):
        with fd.DavidsonEngine(a.shape[0], lowest) as eng:
            eng.set_sparse(1, *arrays, diagonals=diagonals)
            lam, vec, its[diagonals] = eng.solve(method, CI.MAX_ITERATIONS, 1e-8)
        assert its[diagonals] <= CI.MAX_ITERATIONS, (name, method, its)
        check_pairs(a, None, lam, vec, ev[:lowest])
    print(f"{name} {method}: iterations CSR {its[False]}, by diagonals {its[True]}")


def test_generalized_solve_with_a_by_diagonals_and_a_banded_b():
    n, lowest = 1200, 3
    a = np.diag(1.0 + np.arange(n, dtype=np.float64))
    b = np.eye(n)
    for off, wa, wb in ((1, 0.3, 0.05), (2, 0.15, 0.025)):
        a += wa * (np.eye(n, k=off) + np.eye(n, k=-off))
        b += wb * (np.eye(n, k=off) + np.eye(n, k=-off))
    l = np.linalg.cholesky(b)
    ref = np.linalg.eigvalsh(np.linalg.solve(l, np.linalg.solve(l, a).T))[:lowest]
    its = []
    for a_flag, b_flag in ((False, False), (True, False), (True, True)):
        with fd.DavidsonEngine(n, lowest, gev=True) as eng:
            eng.set_sparse(1, *D.csr_of_dense(a), diagonals=a_flag)
            eng.set_sparse(2, *D.csr_of_dense(b), diagonals=b_flag)
            lam, vec, it = eng.solve("DPR", 300, 1e-8)
        assert it < 300
        its.append(it)
        check_pairs(a, b, lam, vec, ref)
    print(f"generalized DPR: iterations CSR/CSR {its[0]}, DIA/CSR {its[1]}, DIA/DIA {its[2]}")


@pytest.mark.parametrize("option", ["unconverged", "locking", "device_rr", "warm_start"])
def test_policies_device_rayleigh_ritz_and_warm_start(option):
    a, arrays, ev = solve_matrix("lap16")
    lowest = 4
    with fd.DavidsonEngine(a.shape[0], lowest) as eng:
        eng.set_sparse(1, *arrays, diagonals=True)
        if option == "device_rr":
            eng.set_device_rr(True)
        elif option != "warm_start":
            eng.set_correction_policy(option)
        lam, vec, it = eng.solve("CHEB", CI.MAX_ITERATIONS, 1e-8, reuse_vectors=True if option == "warm_start" else None)
        assert it <= CI.MAX_ITERATIONS
        check_pairs(a, None, lam, vec, ev[:lowest])
        if option == "warm_start":
            lam2, vec2, it2 = eng.solve("CHEB12", CI.MAX_ITERATIONS, 1e-8)
            check_pairs(a, None, lam2, vec2, ev[:lowest])
            assert it2 <= 2 < it, (it, it2)


def test_front_ends_take_the_keyword():
    import scipy.sparse as sp
    import torch
    a, arrays, ev = solve_matrix("lap16")
    lowest = 4
    lam, vec, it = fd.solver.generalized_eigensolver_sparse(*arrays, lowest, "CHEB", 300, 1e-8, diagonals=True)
    assert it <= 300
    check_pairs(a, None, lam, vec, ev[:lowest])
    lam, vec, it = fd.solver.generalized_eigensolver_sparse(*D.csr_of_dense(a, lower=True), lowest, "DPR", 400, 1e-8, lower=True, diagonals=True)
    assert it <= 400
    check_pairs(a, None, lam, vec, ev[:lowest])
    dia = sp.dia_matrix(a)
    dev = torch.sparse_csr_tensor(torch.tensor(arrays[0]), torch.tensor(arrays[1].astype(np.int64)), torch.tensor(arrays[2]),
                                  size=a.shape).to("cuda")
    results = []
    for operand in (arrays, (dia,), (dev,)):
        with fd.DavidsonEngine(a.shape[0], lowest) as eng:
            eng.set_sparse(1, *operand, diagonals=True)
            lam, vec, it = eng.solve("CHEB", CI.MAX_ITERATIONS, 1e-8)
        check_pairs(a, None, lam, vec, ev[:lowest])
        results.append((lam, it))
    for lam, it in results[1:]:
        assert it == results[0][1] and same_bits(lam, results[0][0])
    # a matrix that does not suit the storage is refused through the front end too (the device door returns the engine's status), never
    # stored as CSR: the operator is unset, and the engine takes the next matrix
    wild = sp.csr_matrix(CI.random_sparse(256, 6 / 256, 1))
    wild_dev = torch.sparse_csr_tensor(torch.tensor(wild.indptr.astype(np.int64)), torch.tensor(wild.indices.astype(np.int64)),
                                       torch.tensor(wild.data), size=wild.shape).to("cuda")
    with fd.DavidsonEngine(a.shape[0], lowest) as eng:
        with pytest.raises(DavidsonHipError, match="DIA_MAX_FILL"):
            eng.set_sparse(1, wild_dev, diagonals=True)
        eng.set_sparse(1, dia, diagonals=True)
        lam, vec, it = eng.solve("CHEB", CI.MAX_ITERATIONS, 1e-8)
    assert it == results[0][1] and same_bits(lam, results[0][0])


# ---- T9: the Fortran program ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang not available")
def test_fortran_program_sets_and_solves_by_diagonals(tmp_path):
    from test_fortran_programs import FC, LIBDIR, MODDIR, SRC, _run
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "prog_dia")
    cmd = [FC, "-O1", "-fopenmp=libiomp5", f"-I{MODDIR}", "-module-dir", str(tmp_path), os.path.join(SRC, "prog_dia.f90"), f"-L{LIBDIR}",
           "-lfortran_davidson_amd", "-ldavidson_hip", f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/conda/lib", "-Wl,-rpath,/opt/conda/lib", "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path)
    assert res.returncode == 0, res.stderr[-3000:]
    rc, out = _run(exe)
    assert rc == 0, out
    checks = re.findall(r"CHECK (\S+) ([TF])", out)
    assert len(checks) == 9 and all(v == "T" for _, v in checks), out
    n = 256
    a = CI.laplacian2d(16)
    i = np.arange(1, n + 1)
    a[np.arange(n), np.arange(n)] = 4.0 + 0.05 * (((37 * i + 11) % 101) / 101.0 - 0.5)
    ref = np.linalg.eigvalsh(a)[:4]
    for label in ("EVALS_ONE_CALL", "EVALS_ENGINE", "EVALS_DEVICE", "EVALS_CHEB"):
        ev = np.array([float(x) for x in re.search(label + r"(.*)", out).group(1).split()])
        assert np.abs(ev - ref).max() < 1e-9, label
