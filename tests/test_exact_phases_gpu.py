"""GPU: the phases of an outer iteration besides the block products - Ritz / residual / DPR, orthogonalisation and projection, restart,
the GJD block MINRES - against exact references, inside write fences.

Parts A - C run on integer data (tests/exact_inputs.py: every partial sum below 2^53, the host's -Y theta and -C M exact), so every
assertion is bit equality with an int64 product, or an intact fence: source panels hold NaN outside the columns a call reads,
destination panels SENTINEL in every column, and whole panels are compared with the expected panel - a lost term, a misplaced column,
a stale operand image, a dropped last row pair or an in-place race changes at least one bit.
  A. dav_ritz_residual_correction_n / _g: X, R (GJD) and the DPR block T bitwise; the residual norms bitwise np.sqrt of the integer sums
     (narrow set); T with dyadic denominators bitwise under any division, with general integer denominators bitwise numpy's correctly
     rounded R / den and exactly 0 where the denominator is (the den == 0 guard) while the norm still counts R there; padding rows of T
     zero (gram_is_exact); every phase twice in a row with the same bits (the last-workgroup counter is re-armed); a small Y after a
     large one in one engine; lazy Ritz vectors; dav_panel_select; 2 and 3 ranks.  6145 and 8321 rows reach norm_finish_kernel.
  B. dav_ortho_gram, dav_ortho_apply (in place up to 64 columns, through the scratch panel above), dav_ortho_apply_all (the batched
     launch over 2 and 3 panels), dav_project_ortho (the multi launch of gram_kernel) and dav_project into NaN-filled H, S.
  C. dav_restart in place (keep <= 64), through the scratch panel above, keep == m; columns >= keep bit-unchanged.
  D. dav_gjd_correction_n at 1, 2 and 5 inner steps (inner_tol = 0) against exact_inputs.gjd_restatement in long double:
     max_j ||T_j - T_ld,j||_inf / ||T_ld,j||_inf <= 8 gamma(n).  gamma(n) bounds the rounding of each scalar (dot products over n
     terms of well-separated data, in an order that differs between the kernels and numpy); the factor 8 covers at most 5 steps of
     recurrences fed by those scalars.  Each case first asserts that the float64 run of the same restatement lies within gamma(n) of
     the long-double one (the reference alone is inside the condition).  max_inner = 0, zero right-hand sides (the 8- and 16-column
     ranges), ncols < mbasis, the preconditioner's 1e-10 floor (one step: from two steps on the floor case is ill-conditioned), 2 ranks.
     Measured on MI355X: the engine's error is at most 0.035 of the bar (GJD_MEASURED_WORST: the generalized floor case; 0.031 on
     the n x m x steps grid, n = 255, m = 17, two steps; at most 0.021 for n >= 4095).
DISPATCH names the kernel instantiations this module is meant to launch; profiles/exact_phases_kernel_coverage.csv is a rocprofv3 kernel
trace of one run of it, and tests/test_exact_phases_coverage.py checks the two against each other."""
import zlib

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import (METHOD_CHEB, METHOD_DPR, METHOD_GJD, METHOD_LCHEB, METHOD_NONE, OP_A, OP_B, PANEL_BV, PANEL_R, PANEL_V,
                                           PANEL_W, PANEL_X, method_cheb, method_lcheb)
import cheb_inputs as CI
from exact_inputs import (SENTINEL, GjdInputs, cols_alloc, dpr_diagonals, dpr_reference, fenced, gamma, gjd_error, gram_is_exact,
                          int_block, int_matrix, int_product, mismatch, ritz_inputs, ritz_reference, run_ranks, same_bits, unit_block)

pytestmark = pytest.mark.gpu

# error / (8 gamma(n)) of the engine, the worst over every part D case, measured on MI355X (each case prints its own)
GJD_MEASURED_WORST = 0.035


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _engine(n, max_cols, gev=False, **kw):
    e = fd.CEngine(n=n, max_cols=max_cols, gev=gev, **kw)
    e.cols = cols_alloc(max_cols)
    return e


def _compare(msgs, what, got, exp):
    if not same_bits(got, exp):
        msgs.append(f"{what}: {mismatch(got, exp)}")


# ---- A. Ritz / residual / DPR ----------------------------------------------------------------------------------------------------------
RITZ_SHAPES = [(1, 1, 1), (6, 6, 3), (12, 5, 2), (33, 17, 17), (64, 40, 9), (128, 100, 70)]       # m, ncorr, lowest
RITZ_NS = [1, 255, 1027, 2305]
RITZ_LARGE = [(6145, (12, 5, 2)), (6145, (33, 17, 17)), (8321, (12, 5, 2)), (8321, (33, 17, 17))]    # 50 and 66 row blocks of 128
# (kind, method, denominators, entry): wide / narrow data; "dyadic" / "general" denominators of the DPR block; "g": the _g entry
RITZ_RUNS = [("wide", METHOD_GJD, None, "n"), ("narrow", METHOD_GJD, None, "n"), ("wide", METHOD_DPR, "dyadic", "n"),
             ("narrow", METHOD_DPR, "dyadic", "g"), ("narrow", METHOD_DPR, "general", "n"), ("wide", METHOD_DPR, "general", "n")]


def ritz_phase(e, n, shape, gev, kind, method, denom, entry, tag, lazy=False, keep=None):
    """One Ritz phase inside fences, twice in a row; returns the messages of everything that is not bit for bit the reference.
    keep: a dict that receives the inputs and the panels after the call."""
    m, ncorr, lowest = shape
    cols = e.cols
    rng = np.random.default_rng(_seed("ritz", n, shape, gev, kind, method, denom, tag))
    dpr = method == METHOD_DPR
    v, w, z, y, theta = ritz_inputs(kind, n, m, ncorr, gev, rng, dyadic=denom == "dyadic")
    xi, ri, ss = ritz_reference(v, w, z, y, theta)
    src = {PANEL_V: fenced(n, cols, SENTINEL if dpr else np.nan, 0, v), PANEL_W: fenced(n, cols, np.nan, 0, w),
           PANEL_X: fenced(n, cols, SENTINEL), PANEL_R: fenced(n, cols, SENTINEL)}
    if gev:
        src[PANEL_BV] = fenced(n, cols, np.nan, 0, z)
    exp = {p: a.copy() for p, a in src.items()}
    if dpr:
        da, db, guard = dpr_diagonals(n, gev, theta, rng, None if denom == "dyadic" else lowest - 1)
        e.set_operator_host(OP_A, da)
        if gev:
            e.set_operator_host(OP_B, db)
        t, den = dpr_reference(ri, theta, da, db)
        exp[PANEL_V][:, m:m + ncorr] = t
        if not lazy:
            exp[PANEL_X][:, :lowest] = xi[:, :lowest]
    else:
        exp[PANEL_R][:, :ncorr] = ri
        exp[PANEL_X][:, :ncorr] = xi
    for p, a in src.items():
        e.panel_put(p, 0, a)
    runs = []
    for _ in range(2):
        if entry == "g":
            out = e.ritz_residual_correction_g(m, ncorr, lowest, y, theta)
        else:
            out = (e.ritz_residual_correction_n(m, ncorr, lowest, y, theta, method),)
        runs.append((out, {p: e.panel_get(p, 0, cols) for p in src}))
    msgs = []
    (out, got), (out2, got2) = runs
    for p in src:
        _compare(msgs, f"panel {p}", got[p], exp[p])
        _compare(msgs, f"panel {p}, second call against the first", got2[p], got[p])
    for a, b in zip(out, out2):
        _compare(msgs, "small results, second call against the first", b, a)
    if kind == "narrow":
        assert (ss < 2 ** 53).all()
        _compare(msgs, "residual norms", out[0], np.sqrt(ss[:lowest].astype(np.float64)))
    if dpr and denom == "general":
        assert (t[guard, lowest - 1] == 0.0).all() and (den[guard, lowest - 1] == 0.0).all()
        if not (got[PANEL_V][guard, m + lowest - 1] == 0.0).all():
            msgs.append("T is not exactly 0 where the denominator is")
    if dpr and denom == "dyadic" and kind == "narrow":
        if not gram_is_exact(e.gram(PANEL_V, m, ncorr, PANEL_V, m, ncorr), t):
            msgs.append("gram(T, T) != T^T T: padding rows of T are not zero")
    if entry == "g":
        _compare(msgs, "C = V^T T", out[1], np.asfortranarray(v.T @ t))           # unit entries times multiples of 2^-3: exact
        _compare(msgs, "G = T^T T", out[2], np.asfortranarray(t.T @ t))
    if keep is not None:
        keep.update(v=v, y=y, theta=theta, xi=xi, t=t if dpr else None, got=got2, exp=exp, res=out[0])
    return [f"{kind} {'DPR' if dpr else 'GJD'} {denom} {shape} gev={gev} {tag}: {s}" for s in msgs]


def _ritz_all_runs(n, shape, max_cols=None):
    msgs = []
    for gev in (False, True):
        with _engine(n, max_cols or shape[0] + shape[1], gev) as e:
            for kind, method, denom, entry in RITZ_RUNS:
                msgs += ritz_phase(e, n, shape, gev, kind, method, denom, entry, "")
    return msgs


@pytest.mark.parametrize("shape", RITZ_SHAPES, ids=lambda s: "m%d-c%d-l%d" % s)
@pytest.mark.parametrize("n", RITZ_NS)
def test_ritz_residual_dpr_phase_is_exact_and_fenced(n, shape):
    msgs = _ritz_all_runs(n, shape)
    assert not msgs, msgs


@pytest.mark.parametrize("n,shape", RITZ_LARGE, ids=lambda v: str(v).replace(" ", ""))
def test_ritz_phase_with_norm_finish_kernel_is_exact(n, shape):
    """more than PG_FUSE_BLOCKS = 48 row blocks: the norms are summed by norm_finish_kernel (66 blocks: its lanes stride twice)"""
    msgs = _ritz_all_runs(n, shape)
    assert not msgs, msgs


@pytest.mark.parametrize("pin", ["1", "0"])
@pytest.mark.parametrize("shape", [(12, 5, 2), (33, 17, 17), (64, 40, 9), (128, 100, 70)], ids=lambda s: "m%d-c%d-l%d" % s)
def test_ritz_phase_is_exact_with_either_schedule(shape, pin, monkeypatch):
    monkeypatch.setenv("DAV_PG_PIN", pin)
    msgs = _ritz_all_runs(1027, shape)
    assert not msgs, msgs


def test_small_ritz_phase_after_a_large_one_sees_no_stale_operand_image():
    n, big, small = 1027, (128, 100, 70), (6, 6, 3)
    msgs = []
    for gev in (False, True):
        with _engine(n, big[0] + big[1], gev) as e:
            for kind, method, denom, entry in RITZ_RUNS:
                msgs += ritz_phase(e, n, big, gev, kind, method, denom, entry, "large first")
                msgs += ritz_phase(e, n, small, gev, kind, method, denom, entry, "then small")
                msgs += ritz_phase(e, n, (33, 17, 17), gev, kind, method, denom, entry, "then medium")
    assert not msgs, msgs


@pytest.mark.parametrize("shape", [(12, 5, 2), (64, 40, 9)], ids=lambda s: "m%d-c%d-l%d" % s)
def test_lazy_ritz_vectors_leave_x_alone_until_asked(shape):
    n = 1027
    m, ncorr, lowest = shape
    with _engine(n, m + ncorr) as e:
        e.set_lazy_ritz_vectors(True)
        k = {}
        msgs = ritz_phase(e, n, shape, False, "wide", METHOD_DPR, "dyadic", "n", "lazy", lazy=True, keep=k)
        assert not msgs, msgs                                  # X is all sentinel, T and the rest as ever
        e.ritz_vectors(m, lowest, k["y"])
        x = e.panel_get(PANEL_X, 0, e.cols)
        exp = fenced(n, e.cols, SENTINEL, 0, k["xi"][:, :lowest].astype(np.float64))
        assert same_bits(x, exp), mismatch(x, exp)
        assert same_bits(e.panel_get(PANEL_V, 0, e.cols), k["exp"][PANEL_V])
        e.set_lazy_ritz_vectors(False)
        msgs = ritz_phase(e, n, shape, False, "wide", METHOD_DPR, "dyadic", "n", "eager again")
        assert not msgs, msgs


def test_panel_select_moves_the_chosen_columns_bitwise_and_nothing_else():
    n, shape = 1027, (33, 17, 17)
    m, ncorr, _ = shape
    with _engine(n, m + ncorr) as e:
        k = {}
        msgs = ritz_phase(e, n, shape, False, "wide", METHOD_DPR, "general", "n", "select", keep=k)
        assert not msgs, msgs
        w_before = e.panel_get(PANEL_W, 0, e.cols)
        for sel in ([0, 1, 2], [0, 2, 5, 16], [3], [1, 4, 7, 8, 9, 15]):
            before = e.panel_get(PANEL_V, 0, e.cols)
            exp = before.copy()
            for i, s in enumerate(sel):
                exp[:, m + i] = exp[:, m + s]                # ascending, to the left: as the engine does it
            e.panel_select(PANEL_V, m, sel)
            after = e.panel_get(PANEL_V, 0, e.cols)
            assert same_bits(after, exp), (sel, mismatch(after, exp))
        assert same_bits(e.panel_get(PANEL_W, 0, e.cols), w_before)


RITZ_RANK_RUNS = [("wide", METHOD_GJD, None, "n"), ("narrow", METHOD_DPR, "dyadic", "g"), ("narrow", METHOD_DPR, "general", "n"),
                  ("wide", METHOD_DPR, "dyadic", "n")]


@pytest.mark.parametrize("nranks", [2, 3])
def test_ritz_phase_is_exact_over_ranks(nranks):
    """the references do not depend on the rank count, so bits that match them match the one-rank result"""
    n, shape, gev = 1027, (33, 17, 17), True

    def work(r, e):
        e.cols = cols_alloc(shape[0] + shape[1])
        msgs = []
        for kind, method, denom, entry in RITZ_RANK_RUNS:
            msgs += ritz_phase(e, n, shape, gev, kind, method, denom, entry, "")
        return msgs
    outs = run_ranks(nranks, lambda r: fd.CEngine(n=n, max_cols=shape[0] + shape[1], gev=gev, rank=r, nranks=nranks), work)
    for msgs in outs:
        assert not msgs, msgs


# ---- A2. the method code ------------------------------------------------------------------------------------------------------------------
def test_a_method_code_is_split_once_and_a_code_that_names_no_method_corrects_nothing():
    """The Ritz phase of a CSR operator (n = 240, m = ncorr = 5, lowest = 4) under method codes that must mean the same: CHEB and LCHEB
    without a degree are degree 10 bit for bit (norms, R, T).  A code that names no method - a degree above a low byte that takes none,
    and a low byte no method has - is not refused: the phase returns 0, writes R and the norms as DAV_METHOD_NONE does and leaves the
    columns of the correction block alone."""
    n, m, lowest = 240, 5, 4
    a = CI.random_sparse(n, 6.0 / n, 3, grade=0.5 / n)
    v = np.asfortranarray(np.linalg.qr(np.random.default_rng(4).standard_normal((n, m)))[0])
    w = np.asfortranarray(a @ v)
    theta, y = np.linalg.eigh(v.T @ w)
    mark = np.full((n, m), 3.25)

    def phase(e, method):
        e.panel_put(PANEL_V, m, mark)
        e.panel_put(PANEL_R, 0, mark)
        e.panel_put(PANEL_V, 0, v)
        e.panel_put(PANEL_W, 0, w)
        norms = e.ritz_residual_correction(m, lowest, y, theta, method)
        return norms.reshape(1, -1), e.panel_get(PANEL_R, 0, m), e.panel_get(PANEL_V, m, m)

    msgs = []
    with fd.CEngine(n=n, max_cols=16) as e:
        e.set_operator_csr(OP_A, *CI.csr_of(a))
        none = phase(e, METHOD_NONE)
        assert not same_bits(none[1], mark) and same_bits(none[2], mark) and np.isfinite(none[0]).all()
        for name, default, ten, three in (("CHEB", METHOD_CHEB, method_cheb(10), method_cheb(3)),
                                          ("LCHEB", METHOD_LCHEB, method_lcheb(10), method_lcheb(3))):
            got, want, other = phase(e, default), phase(e, ten), phase(e, three)
            for what, g, x in zip(("norms", "R", "T"), got, want):
                _compare(msgs, f"{name} without a degree against degree 10, {what}", g, x)
            _compare(msgs, f"{name}, R against DAV_METHOD_NONE's", got[1], none[1])
            assert not same_bits(got[2], mark) and not same_bits(got[2], other[2]), name      # a block was written, and the degree counts
        for code in (METHOD_DPR | 7 << 8, 6):
            got = phase(e, code)
            _compare(msgs, f"code {code}, norms against DAV_METHOD_NONE's", got[0], none[0])
            _compare(msgs, f"code {code}, R against DAV_METHOD_NONE's", got[1], none[1])
            _compare(msgs, f"code {code}, the columns of the correction block", got[2], mark)
    assert not msgs, msgs


# ---- B. orthogonalisation and projection ------------------------------------------------------------------------------------------------
ORTHO_SHAPES = [(0, 1), (0, 9), (5, 17), (33, 40), (64, 64), (20, 80)]          # m, kt
ORTHO_APPLY_SHAPES = ORTHO_SHAPES + [(12, 65)]                                 # kt <= 64 in place; 65 and 80 through the scratch panel
ORTHO_NS = [255, 2305]


def _basis_panel(n, cols, m, kt, rng, fill, v=None, t=None):
    """[V T] in the columns 0 .. m + kt of a panel of `fill`: V from unit_block, T from int_block(bits=20) unless given"""
    v = unit_block(n, m, rng) if v is None else v
    t = int_block(n, kt, rng, bits=20) if t is None else t
    p = fenced(n, cols, fill, 0, v)
    p[:, m:m + kt] = t
    return p, v, t


def ortho_gram_case(e, n, m, kt):
    cols = e.cols
    rng = np.random.default_rng(_seed("ortho gram", n, m, kt))
    p, v, t = _basis_panel(n, cols, m, kt, rng, np.nan)
    nan = fenced(n, cols, np.nan)
    e.panel_put(PANEL_V, 0, p)
    e.panel_put(PANEL_W, 0, nan)
    c, g = e.ortho_gram(m, kt)
    msgs = []
    _compare(msgs, "C = V^T T", c, np.asfortranarray(int_product(v.T, t).astype(np.float64)))
    _compare(msgs, "G = T^T T", g, np.asfortranarray(int_product(t.T, t).astype(np.float64)))
    _compare(msgs, "V panel", e.panel_get(PANEL_V, 0, cols), p)
    _compare(msgs, "W panel", e.panel_get(PANEL_W, 0, cols), nan)
    return [f"ortho_gram n={n} m={m} kt={kt}: {s}" for s in msgs]


def ortho_apply_case(e, n, m, kt, gev, with_images):
    """T <- T M + V (-C M) in place (and the same on W, B V with their own leading columns), integer C and M"""
    cols = e.cols
    rng = np.random.default_rng(_seed("ortho apply", n, m, kt, gev, with_images))
    c, mm = int_matrix(m, kt, rng), int_matrix(kt, kt, rng)
    cm = -int_product(c, mm)                                                    # the host's -C M, exact
    panels = [PANEL_V] + ([PANEL_W] + ([PANEL_BV] if gev else []) if with_images else [])
    idle = [p for p in ([PANEL_W] + ([PANEL_BV] if gev else [])) if p not in panels]
    src, exp = {}, {}
    for p in panels:
        lead = unit_block(n, m, rng) if p == PANEL_V else int_block(n, m, rng, bits=20)
        src[p], lead, t = _basis_panel(n, cols, m, kt, rng, SENTINEL, v=lead)
        exp[p] = src[p].copy()
        exp[p][:, m:m + kt] = int_product(t, mm) + lead.astype(np.int64) @ cm
    for p in idle:
        src[p] = exp[p] = fenced(n, cols, np.nan)
    for p, a in src.items():
        e.panel_put(p, 0, a)
    (e.ortho_apply_all if with_images else e.ortho_apply)(m, kt, c, mm)
    msgs = []
    for p in src:
        _compare(msgs, f"panel {p}", e.panel_get(p, 0, cols), exp[p])
    return [f"ortho_apply{'_all' if with_images else ''} n={n} m={m} kt={kt} gev={gev}: {s}" for s in msgs]


@pytest.mark.parametrize("n", ORTHO_NS)
def test_ortho_gram_is_exact_and_leaves_the_panels_alone(n):
    msgs = []
    with _engine(n, 112) as e:
        for m, kt in ORTHO_SHAPES:
            msgs += ortho_gram_case(e, n, m, kt)
    assert not msgs, msgs


@pytest.mark.parametrize("gev", [False, True])
@pytest.mark.parametrize("n", ORTHO_NS)
def test_ortho_apply_is_exact_in_place_and_fenced(n, gev):
    msgs = []
    with _engine(n, 112, gev) as e:
        for m, kt in ORTHO_APPLY_SHAPES:
            msgs += ortho_apply_case(e, n, m, kt, gev, False)
    assert not msgs, msgs


@pytest.mark.parametrize("pin", ["1", "0"])
@pytest.mark.parametrize("gev", [False, True])
@pytest.mark.parametrize("n", ORTHO_NS)
def test_ortho_apply_all_carries_the_images_exactly(n, gev, pin, monkeypatch):
    """2 panels (standard) and 3 (generalized) in one batched launch up to 64 columns, one launch per panel through the scratch above"""
    monkeypatch.setenv("DAV_PG_PIN", pin)
    msgs = []
    with _engine(n, 112, gev) as e:
        for m, kt in ORTHO_APPLY_SHAPES:
            msgs += ortho_apply_case(e, n, m, kt, gev, True)
    assert not msgs, msgs


def project_ortho_case(e, n, m, k, gev):
    cols = e.cols
    rng = np.random.default_rng(_seed("project ortho", n, m, k, gev))
    pv, v, t = _basis_panel(n, cols, m, k, rng, np.nan)
    src = {PANEL_V: pv, PANEL_W: fenced(n, cols, np.nan, m, int_block(n, k, rng, bits=20))}
    if gev:
        src[PANEL_BV] = fenced(n, cols, np.nan, m, int_block(n, k, rng, bits=20))
    for p, a in src.items():
        e.panel_put(p, 0, a)
    h, s, c, g = e.project_ortho(m, k, gev)
    vt = pv[:, :m + k]
    msgs = []
    _compare(msgs, "H_raw", h, np.asfortranarray(int_product(vt.T, src[PANEL_W][:, m:m + k]).astype(np.float64)))
    if gev:
        _compare(msgs, "S_raw", s, np.asfortranarray(int_product(vt.T, src[PANEL_BV][:, m:m + k]).astype(np.float64)))
    _compare(msgs, "C", c, np.asfortranarray(int_product(v.T, t).astype(np.float64)))
    _compare(msgs, "G", g, np.asfortranarray(int_product(t.T, t).astype(np.float64)))
    for p in src:
        _compare(msgs, f"panel {p}", e.panel_get(p, 0, cols), src[p])
    return [f"project_ortho n={n} m={m} k={k} gev={gev}: {s}" for s in msgs]


def project_case(e, n, c0, k, gev):
    """dav_project into H (and S) prefilled with NaN: the new columns and their mirror are V^T W, every other entry is still NaN"""
    cols = e.cols
    mt = c0 + k
    rng = np.random.default_rng(_seed("project", n, c0, k, gev))
    src = {PANEL_V: fenced(n, cols, np.nan, 0, int_block(n, mt, rng, bits=20)),
           PANEL_W: fenced(n, cols, np.nan, c0, int_block(n, k, rng, bits=20))}
    if gev:
        src[PANEL_BV] = fenced(n, cols, np.nan, c0, int_block(n, k, rng, bits=20))
    for p, a in src.items():
        e.panel_put(p, 0, a)
    h = np.full((mt + 3, mt + 3), np.nan, order="F")
    s = np.full((mt + 3, mt + 3), np.nan, order="F") if gev else None
    e.project(c0, k, h, s)
    msgs = []
    for name, got, p in (("H", h, PANEL_W), ("S", s, PANEL_BV))[:2 if gev else 1]:
        blk = int_product(src[PANEL_V][:, :mt].T, src[p][:, c0:mt]).astype(np.float64)
        exp = np.full_like(got, np.nan)
        exp[:mt, c0:mt] = blk
        exp[c0:mt, :c0] = blk[:c0].T
        _compare(msgs, name, got, exp)
    for p in src:
        _compare(msgs, f"panel {p}", e.panel_get(p, 0, cols), src[p])
    return [f"project n={n} c0={c0} k={k} gev={gev}: {s}" for s in msgs]


@pytest.mark.parametrize("gev", [False, True])
@pytest.mark.parametrize("n", ORTHO_NS)
def test_project_ortho_and_project_are_exact(n, gev):
    msgs = []
    with _engine(n, 80, gev) as e:
        for m, k in ((5, 17), (33, 40)):
            msgs += project_ortho_case(e, n, m, k, gev)
        for c0, k in ((0, 6), (8, 8), (33, 17)):
            msgs += project_case(e, n, c0, k, gev)
    assert not msgs, msgs


def test_orthogonalisation_is_exact_over_three_ranks():
    n, gev = 2305, True

    def work(r, e):
        e.cols = cols_alloc(112)
        msgs = ortho_gram_case(e, n, 33, 40)
        for m, kt in ((33, 40), (12, 65)):
            msgs += ortho_apply_case(e, n, m, kt, gev, True)
        return msgs + project_ortho_case(e, n, 5, 17, gev) + project_case(e, n, 33, 17, gev)
    for msgs in run_ranks(3, lambda r: fd.CEngine(n=n, max_cols=112, gev=gev, rank=r, nranks=3), work):
        assert not msgs, msgs


# ---- C. restart -------------------------------------------------------------------------------------------------------------------------
RESTART_SHAPES = [(12, 1), (33, 8), (128, 64), (128, 65), (100, 100)]           # m, keep: in place up to 64, through scratch, keep == m


@pytest.mark.parametrize("gev", [False, True])
@pytest.mark.parametrize("n", [257, 2305])
def test_restart_is_exact_and_leaves_the_other_columns_alone(n, gev):
    msgs = []
    with _engine(n, 128, gev) as e:
        cols = e.cols
        for m, keep in RESTART_SHAPES:
            rng = np.random.default_rng(_seed("restart", n, m, keep, gev))
            yk = int_matrix(m, keep, rng)
            src, exp = {}, {}
            for p in [PANEL_V, PANEL_W] + ([PANEL_BV] if gev else []):
                blk = int_block(n, m, rng, bits=20)
                src[p] = fenced(n, cols, np.nan, 0, blk)
                exp[p] = src[p].copy()
                exp[p][:, :keep] = int_product(blk, yk)
            for p, a in src.items():
                e.panel_put(p, 0, a)
            e.restart(m, keep, yk)
            for p in src:
                _compare(msgs, f"restart n={n} m={m} keep={keep} gev={gev}, panel {p}", e.panel_get(p, 0, cols), exp[p])
            assert e.stats().m == keep
    assert not msgs, msgs


# ---- D. the GJD correction at fixed step counts --------------------------------------------------------------------------------------------
GJD_NS = [255, 4095, 4097, 8321]          # 1, 1, 2 and 3 blocks of coldots_kernel (DOT_ROWS = 4096 padded rows)
GJD_MS = [1, 3, 9, 17]
GJD_STEPS = [1, 2, 5]
# name -> (n, mbasis, ncols, gev, steps, keyword arguments of GjdInputs): the cases besides the n x m x gev grid
GJD_SPECIAL = {
    "one-nonzero-column": (4097, 17, 17, False, (1, 2, 5), dict(zero_cols=tuple(range(16)))),          # the 8-column range
    "nine-zero-columns": (4097, 17, 17, True, (1, 2, 5), dict(zero_cols=tuple(range(9)))),             # the 16-column groups
    "narrower-than-the-basis": (4097, 12, 5, True, (1, 2, 5), {}),
    "floor": (4097, 9, 9, False, (1,), dict(floor=True)),
    "floor-generalized": (255, 3, 3, True, (1,), dict(floor=True)),
}
_ZERO16, _ZERO9 = (("zero_cols", tuple(range(16))),), (("zero_cols", tuple(range(9))),)
# The seed of a case is the first of 0, 1, 2, .. for which the float64 restatement lies within gamma(n) / 2 of the long-double one at
# every step count of the case - a property of the reference alone; 0 unless listed.  Columns with theta_j >= 1 (j >= 10) lie inside
# the range of diag(A): where a draw puts a diagonal entry within 1e-4 .. 1e-3 of theta_j dB_i, the projection y + cy K^-1 x cancels a
# spike of K^-1 and the recurrences lose that many digits in float64 as well - such a draw tests the conditioning, not the kernels.
GJD_SEEDS = {(255, 17, False, ()): 1, (255, 17, True, ()): 37, (4095, 17, False, ()): 1, (4095, 17, True, ()): 10, (4097, 17, False, ()): 4,
             (4097, 17, True, ()): 8, (8321, 17, False, ()): 3, (8321, 17, True, ()): 4, (4097, 17, False, _ZERO16): 3,
             (4097, 17, True, _ZERO9): 8}
_GJD_REFS = {}


def gjd_inputs(n, m, gev, **kw):
    return GjdInputs(n, m, gev, GJD_SEEDS.get((n, m, gev, tuple(sorted(kw.items()))), 0), **kw)


def gjd_references(n, m, gev, steps, **kw):
    """(inputs, T in long double, error of the float64 restatement against it) - computed once per case"""
    key = (n, m, gev, steps, repr(sorted(kw.items())))
    if key not in _GJD_REFS:
        inp = gjd_inputs(n, m, gev, **kw)
        t_ld, it = inp.restate(steps, np.longdouble)
        t_64, it64 = inp.restate(steps, np.float64)
        assert it == it64 == steps
        _GJD_REFS[key] = (inp, t_ld, gjd_error(t_64, t_ld))
    return _GJD_REFS[key]


def gjd_grid_cases():
    return [(n, m, gev, s, {}) for n in GJD_NS for m in GJD_MS for gev in (False, True) for s in GJD_STEPS]


def gjd_all_cases():
    return gjd_grid_cases() + [(n, nc, gev, s, kw) for n, _, nc, gev, steps, kw in GJD_SPECIAL.values() for s in steps]


def gjd_run(e, inp, mbasis, steps):
    """dav_gjd_correction_n inside fences: (T, steps taken, messages about the columns and panels the call must leave alone)"""
    n, m, cols = inp.n, inp.m, e.cols
    src = {PANEL_V: fenced(n, cols, SENTINEL), PANEL_X: fenced(n, cols, np.nan, 0, inp.x), PANEL_R: fenced(n, cols, SENTINEL, 0, inp.r)}
    for p, a in src.items():
        e.panel_put(p, 0, a)
    its = e.gjd_correction_steps(mbasis, m, inp.theta, steps)
    got = {p: e.panel_get(p, 0, cols) for p in src}
    msgs = []
    _compare(msgs, "X panel", got[PANEL_X], src[PANEL_X])
    _compare(msgs, "R panel beyond the right-hand sides", got[PANEL_R][:, m:], src[PANEL_R][:, m:])
    outside = np.ones(cols, dtype=bool)
    outside[mbasis:mbasis + m] = False
    _compare(msgs, "V panel outside T", got[PANEL_V][:, outside], src[PANEL_V][:, outside])
    if steps == 0:
        _compare(msgs, "R panel = -R", got[PANEL_R][:, :m], -inp.r)
    return np.asfortranarray(got[PANEL_V][:, mbasis:mbasis + m]), its, msgs


def gjd_check(tag, t, its, msgs, ref, steps):
    """the reference is inside the condition; the engine took `steps` steps, left its fences alone, and T is within 8 gamma(n)"""
    inp, t_ld, err64 = ref
    assert err64 <= gamma(inp.n), (tag, "the float64 restatement is not within gamma(n) of the long-double one", err64 / gamma(inp.n))
    assert not msgs, (tag, msgs)
    assert its == steps, (tag, its)
    zero = ~inp.r.any(axis=0)
    assert (t[:, zero] == 0.0).all(), (tag, "a zero right-hand side has a nonzero correction")
    assert not (t_ld[:, zero] != 0).any()
    err = gjd_error(t, t_ld)
    print(f"gjd {tag}: error / (8 gamma(n)) = {err / (8 * gamma(inp.n)):.4f}, float64 restatement / gamma(n) = {err64 / gamma(inp.n):.4f}")
    assert err <= 8 * gamma(inp.n), (tag, err / (8 * gamma(inp.n)))


@pytest.mark.parametrize("gev", [False, True])
@pytest.mark.parametrize("m", GJD_MS)
@pytest.mark.parametrize("n", GJD_NS)
def test_gjd_correction_matches_the_long_double_restatement(n, m, gev):
    with _engine(n, 2 * m + 2, gev) as e:
        gjd_inputs(n, m, gev).set_operators(e)
        for steps in GJD_STEPS:
            ref = gjd_references(n, m, gev, steps)
            t, its, msgs = gjd_run(e, ref[0], m, steps)
            gjd_check(f"n={n} m={m} gev={gev} steps={steps}", t, its, msgs, ref, steps)


@pytest.mark.parametrize("name", list(GJD_SPECIAL))
def test_gjd_correction_special_cases(name):
    n, mbasis, ncols, gev, steps_list, kw = GJD_SPECIAL[name]
    with _engine(n, mbasis + ncols + 2, gev) as e:
        gjd_inputs(n, ncols, gev, **kw).set_operators(e)
        for steps in steps_list:
            ref = gjd_references(n, ncols, gev, steps, **kw)
            t, its, msgs = gjd_run(e, ref[0], mbasis, steps)
            gjd_check(f"{name} steps={steps}", t, its, msgs, ref, steps)


@pytest.mark.parametrize("gev", [False, True])
def test_gjd_correction_with_no_inner_steps_is_exact(gev):
    n, m = 4097, 9
    inp = gjd_inputs(n, m, gev)
    with _engine(n, 2 * m + 2, gev) as e:
        inp.set_operators(e)
        t, its, msgs = gjd_run(e, inp, m, 0)
    assert not msgs, msgs
    assert its == 0
    assert same_bits(t, np.zeros((n, m), order="F")), mismatch(t, np.zeros((n, m)))


def test_gjd_correction_matches_the_restatement_over_two_ranks():
    n, m, gev, steps = 4097, 9, True, 2
    ref = gjd_references(n, m, gev, steps)

    def work(r, e):
        e.cols = cols_alloc(2 * m + 2)
        ref[0].set_operators(e)
        return gjd_run(e, ref[0], m, steps)
    for t, its, msgs in run_ranks(2, lambda r: fd.CEngine(n=n, max_cols=2 * m + 2, gev=gev, rank=r, nranks=2), work):
        gjd_check("two ranks", t, its, msgs, ref, steps)


# ---- F. the kernels this module is meant to launch ----------------------------------------------------------------------------------------
def _dispatch():
    table = {}
    for qt, what in ((1, "up to 16 output columns: ritz (1,1,1), (6,6,3), (12,5,2); ortho kt = 1, 9; restart keep = 1, 8"),
                     (2, "17 - 32 output columns: ritz (33,17,17); ortho kt = 17"),
                     (4, "33 and more output columns: ritz (64,40,9), (128,100,70); ortho kt = 40 .. 80; restart keep = 64, 65, 100")):
        table[f"panel_gemm_kernel<{qt}, 8, true>"] = [what + ", DAV_PG_PIN=1"]
        table[f"panel_gemm_kernel<{qt}, 8, false>"] = [what + ", DAV_PG_PIN=0"]
    table["norm_finish_kernel"] = ["ritz phases at 6145 and 8321 rows; every coldots of the GJD correction"]
    table["lincomb_kernel"] = table["precond_kernel"] = table["coldots_kernel"] = ["part D"]
    table["copy_columns_kernel"] = ["panel_select; ortho kt = 65, 80 and restart keep = 65, 100 through the scratch panel; part D"]
    table["gram_kernel<4, 4, 4>"] = ["ortho_gram (0,1), (0,9); project (0,6), (8,8); the _g ritz phase of (1,1,1), (6,6,3)"]
    table["gram_kernel<8, 4, 4>"] = ["the _g ritz phase of (12,5,2): 17 x 5"]
    table["gram_kernel<8, 8, 3>"] = ["ortho_gram (5,17) ..; project (33,17); project_ortho (5,17), (33,40): launch_gram_multi, 22 x 34 / 51 .."]
    return table


DISPATCH = _dispatch()
