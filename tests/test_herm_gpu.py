"""Complex Hermitian CSR operators through their real form (davh_set_operator_csr, davh_set_operator_csr_dev; the pair kernels of
fortran_davidson_amd/csrc/k_bsr_build.hip).  The contract: both entries build, bit for bit, the store that
dav_set_operator_bsr(_dev) builds from the same pattern and the numpy-expanded blocks [[a, -b], [b, a]] - so everything downstream serves
a Hermitian operator as it serves any BSR operator with b = 2.
T1 store identity: diagonal and fenced applies as uint64 bits over the six matrix classes, full and lower, both bases, host and device,
   the index widths, the complex orders 1, 17, 300 and 1025, three ranks, slots A, B and M.
T2 exactness: integer (re, im) and integer operands - the product is the int64 complex product.
T3 refusals: every text, host and device equal; the operator is unset afterwards and the next set call works.
T4 refresh: dav_update_operator_values(_dev) with complex values gives the bits of a fresh set call; a real BSR operator is unchanged.
T5 solves at n_c = 200 (the 20 x 20 lattice: 400), lowest 4, tolerance 1e-8, against scipy.linalg.eigh: the one-shot, DavidsonEngine, a tensor on the GPU; the
   methods; the bits of the BSR engine."""
import itertools
import re

import numpy as np
import pytest
import torch

import fortran_davidson_amd as fd
import herm_inputs as H
from exact_inputs import fenced_apply, int_block, run_ranks, same_bits
from fortran_davidson_amd.engine_c import OP_A, OP_B, OP_M, PANEL_V, PANEL_W, DavidsonHipError

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ORDERS = (1, 17, 300, 1025)
COLS = 64
KS = ((1, 0, 0), (17, 1, 3), (64, 0, 0))          # columns, first source column, first destination column
WIDTHS = {"32/32": (torch.int32, torch.int32), "64/64": (torch.int64, torch.int64), "64/32": (torch.int64, torch.int32)}


def to_dev(indptr, indices, data, base=0, rt=torch.int64, ct=torch.int64):
    return (torch.tensor(indptr + base, dtype=rt, device=DEV), torch.tensor(indices + base, dtype=ct, device=DEV),
            torch.tensor(data, device=DEV))


def observe(e, x, which=OP_A):
    """the diagonal and the fenced applies of operator `which`"""
    ap = lambda sp, c0, k, dp, d0: e.apply(which, sp, c0, k, dp, d0)          # noqa: E731
    out, msgs = [e.get_diagonal(which)], []
    for k, c0, d0 in KS:
        w, m = fenced_apply(e, x[:, :k], c0, d0, COLS, ap)
        out.append(w)
        msgs += m
    return out, msgs


def assert_same(got, ref, what):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert same_bits(g, r), (what, k)


# ---- T1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("kind", H.CLASSES)
def test_store_identity_with_the_bsr_entries_on_the_expanded_blocks(kind, lower):
    for nc in ORDERS:
        indptr, indices, data = H.hermitian_csr(nc, kind, lower)
        if kind == "arrowhead" and nc >= 300:
            assert indptr[1] - indptr[0] > 128 or lower          # the first row is longer than BSR_CHUNK: chunks and the finish pass
        blocks = H.expand_blocks(data)
        x = np.random.default_rng(5).standard_normal((2 * nc, COLS))
        with fd.CEngine(n=2 * nc, max_cols=COLS) as eh, fd.CEngine(n=2 * nc, max_cols=COLS) as eb:
            eb.set_operator_bsr(OP_A, indptr, indices, blocks, lower=lower)
            ref, msgs = observe(eb, x)
            assert not msgs, msgs
            for base in (0, 1):
                eh.set_operator_csr_hermitian(OP_A, indptr + base, indices + base, data, base=base, lower=lower)
                got, msgs = observe(eh, x)
                assert not msgs, msgs
                assert_same(got, ref, (nc, "host", base))
            for (name, (rt, ct)), base in itertools.product(WIDTHS.items(), (0, 1)):
                eh.set_operator_csr_hermitian_dev(OP_A, *to_dev(indptr, indices, data, base, rt, ct), base=base, lower=lower)
                got, msgs = observe(eh, x)
                assert not msgs, msgs
                assert_same(got, ref, (nc, "device", name, base))
            # the device BSR entry on the expanded blocks gives the same store too
            rp_d, ci_d, _ = to_dev(indptr, indices, data)
            eb.set_operator_bsr_dev(OP_A, rp_d, ci_d, torch.tensor(blocks, device=DEV), lower=lower)
            assert_same(observe(eb, x)[0], ref, (nc, "bsr device"))


@pytest.mark.parametrize("lower", [False, True])
def test_three_ranks_give_the_bits_of_one_rank(lower):
    nc = 1025
    for kind in ("random", "arrowhead"):
        indptr, indices, data = H.hermitian_csr(nc, kind, lower)
        x = np.random.default_rng(6).standard_normal((2 * nc, COLS))
        with fd.CEngine(n=2 * nc, max_cols=COLS) as e:
            e.set_operator_bsr(OP_A, indptr, indices, H.expand_blocks(data), lower=lower)
            ref, _ = observe(e, x)
        dev = to_dev(indptr, indices, data, 0, torch.int32, torch.int32)

        def work(r, e):
            if r == 1:
                e.set_operator_csr_hermitian(OP_A, indptr, indices, data, lower=lower)
            else:
                e.set_operator_csr_hermitian_dev(OP_A, *dev, lower=lower)
            return observe(e, x)
        outs = run_ranks(3, lambda r: fd.CEngine(n=2 * nc, max_cols=COLS, rank=r, nranks=3), work)
        for r, (got, msgs) in enumerate(outs):
            assert not msgs, msgs
            assert_same(got, ref, (kind, "rank", r))


def test_slots_b_and_m_hold_the_same_store():
    nc = 300
    indptr, indices, data = H.hermitian_csr(nc, "duplicates", True)
    x = np.random.default_rng(7).standard_normal((2 * nc, COLS))
    dev = to_dev(indptr, indices, data)
    with fd.CEngine(n=2 * nc, max_cols=COLS, gev=True) as eh, fd.CEngine(n=2 * nc, max_cols=COLS, gev=True) as eb:
        for which in (OP_B, OP_M):
            eb.set_operator_bsr(which, indptr, indices, H.expand_blocks(data), lower=True)
            ref, _ = observe(eb, x, which)
            eh.set_operator_csr_hermitian(which, indptr, indices, data, lower=True)
            assert_same(observe(eh, x, which)[0], ref, (which, "host"))
            eh.set_operator_csr_hermitian_dev(which, *dev, lower=True)
            assert_same(observe(eh, x, which)[0], ref, (which, "device"))


def test_duplicates_are_summed_in_input_order_and_minus_zero_is_a_real_diagonal():
    """row 0 holds three diagonal terms in two orders - 1, -1, 2^-60 sums to 2^-60 from the left, 1, 2^-60, -1 to 0 - one of them with the
    imaginary part -0.0"""
    indptr = np.array([0, 3, 4], dtype=np.int64)
    indices = np.array([0, 0, 0, 1], dtype=np.int64)
    for terms in ([1.0, -1.0, 2.0 ** -60], [1.0, 2.0 ** -60, -1.0]):
        want = ((0.0 + terms[0]) + terms[1]) + terms[2]
        data = np.array([terms[0], complex(terms[1], -0.0), terms[2], 3.0], dtype=np.complex128)
        for device in (False, True):
            with fd.CEngine(n=4, max_cols=16) as e:
                if device:
                    e.set_operator_csr_hermitian_dev(OP_A, *to_dev(indptr, indices, data))
                else:
                    e.set_operator_csr_hermitian(OP_A, indptr, indices, data)
                assert e.get_diagonal(OP_A).tolist() == [want, want, 3.0, 3.0], (terms, device)


# ---- T2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("kind", H.CLASSES)
def test_integer_products_are_exact(kind, lower):
    for nc in ORDERS:
        indptr, indices, data = H.hermitian_csr(nc, kind, lower, integer=True)
        rng = np.random.default_rng(nc)
        xr, xi = int_block(nc, COLS, rng), int_block(nc, COLS, rng)
        # the int64 complex product H (xr + i xi): |h| <= 255, |x| < 2^28, two products per term, rows of at most 2^11 terms - below 2^49 throughout
        rows = np.repeat(np.arange(nc), np.diff(indptr))
        r, c, a, b = rows, indices, data.real.astype(np.int64), data.imag.astype(np.int64)
        if lower:
            off = rows != indices
            r, c = np.concatenate([rows, indices[off]]), np.concatenate([indices, rows[off]])
            a, b = np.concatenate([a, a[off]]), np.concatenate([b, -b[off]])
        xri, xii = xr.astype(np.int64), xi.astype(np.int64)
        yr, yi = np.zeros((nc, COLS), dtype=np.int64), np.zeros((nc, COLS), dtype=np.int64)
        np.add.at(yr, r, a[:, None] * xri[c] - b[:, None] * xii[c])
        np.add.at(yi, r, b[:, None] * xri[c] + a[:, None] * xii[c])
        want = H.interleave(yr.astype(np.float64) + 1j * yi.astype(np.float64))
        x = H.interleave(xr + 1j * xi)
        for device in (False, True):
            with fd.CEngine(n=2 * nc, max_cols=COLS) as e:
                if device:
                    e.set_operator_csr_hermitian_dev(OP_A, *to_dev(indptr, indices, data), lower=lower)
                else:
                    e.set_operator_csr_hermitian(OP_A, indptr, indices, data, lower=lower)
                got, msgs = observe(e, x)
            assert not msgs, msgs
            for (k, _, _), w in zip(KS, got[1:]):
                assert np.array_equal(w, want[:, :k]), (nc, device, k)


# ---- T3 ------------------------------------------------------------------------------------------------------------------------------
def refusal(e, device, indptr, indices, data, base=0, lower=False, raw=None):
    """the engine's text for a refused set call, without the entry's name; raw: (triangle word, row_ptr_bits, col_bits) for the C call"""
    lib, tri, rpb, cib = e.lib, int(lower), 64, 64
    if raw is not None:
        tri, rpb, cib = raw
    if device:
        rp, ci, vv = to_dev(indptr, indices, data)
        rc = lib.davh_set_operator_csr_dev(e.h, OP_A, rp.data_ptr(), rpb, ci.data_ptr() or None, cib, vv.data_ptr() or None, base, tri)
    else:
        rp, ci, vv = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32), np.asarray(data, dtype=np.complex128)
        rc = lib.davh_set_operator_csr(e.h, OP_A, rp.ctypes.data, ci.ctypes.data if ci.size else None, vv.ctypes.data if vv.size else None,
                                       base, tri)
    assert rc != 0
    text = lib.dav_last_error().decode()
    name = "davh_set_operator_csr_dev: " if device else "davh_set_operator_csr: "
    assert text.startswith(name), text
    return text[len(name):]


def test_every_refusal_host_and_device_alike():
    nc = 17
    indptr, indices, data = H.hermitian_csr(nc, "banded", False)
    rows = np.repeat(np.arange(nc), np.diff(indptr))
    x = np.random.default_rng(8).standard_normal((2 * nc, COLS))
    dpos = np.flatnonzero(rows == indices)

    def decreasing():
        rp = indptr.copy()
        rp[5] = rp[4] - 1
        return rp, indices, data

    def first_offset():
        return indptr + 1, indices, data

    def column_out_of_range():
        ci = indices.copy()
        ci[7] = nc
        return indptr, ci, data

    def imaginary_diagonal():
        vv = data.copy()
        vv[dpos[9]] += 0.5j
        vv[dpos[4]] += 0.25j          # the first offending entry is the one of row 4
        return indptr, indices, vv

    def nan_diagonal():
        vv = data.copy()
        vv[dpos[2]] = complex(vv[dpos[2]].real, np.nan)
        return indptr, indices, vv

    cases = [
        (decreasing, {}, r"row_ptr decreases at row 4$"),
        (first_offset, {}, r"row_ptr\[0\] = 1 must equal the index base 0$"),
        (column_out_of_range, {}, rf"column index {nc} out of range at entry 7 \(row {rows[7]}\)$"),
        (lambda: (indptr, indices, data), {"lower": True}, r"lies above the diagonal of a DAV_CSR_LOWER matrix$"),
        (lambda: (indptr, indices, data), {"base": 2}, r"index_base must be 0 or 1$"),
        (lambda: (indptr, indices, data), {"raw": (4, 64, 64)}, r"triangle must be DAV_CSR_FULL or DAV_CSR_LOWER$"),
        (lambda: (indptr, indices, data), {"raw": (2, 64, 64)}, r"DAV_CSR_DIAGONALS.*a Hermitian operator is stored by blocks$"),
        (imaginary_diagonal, {}, rf"diagonal entry {dpos[4]} \(row 4\) has the imaginary part 0\.25: the diagonal of a Hermitian matrix is real$"),
        (imaginary_diagonal, {"base": 1}, rf"diagonal entry {dpos[4] + 1} \(row 5\) has the imaginary part 0\.25: "),
        (nan_diagonal, {}, rf"diagonal entry {dpos[2]} \(row 2\) has the imaginary part -?nan: "),
    ]
    with fd.CEngine(n=2 * nc, max_cols=COLS) as eh, fd.CEngine(n=2 * nc, max_cols=COLS) as ed:
        for make, kw, pattern in cases:
            rp, ci, vv = make()
            if kw.get("base") == 1:
                rp, ci = rp + 1, ci + 1
            for e in (eh, ed):          # a valid operator with its value map is in place when the call is refused
                e.keep_value_map(OP_A)
                e.set_operator_csr_hermitian(OP_A, indptr, indices, data)
                e.apply(OP_A, PANEL_V, 0, 1, PANEL_W, 0)
            texts = [refusal(e, device, rp, ci, vv, **kw) for e, device in ((eh, False), (ed, True))]
            assert texts[0] == texts[1], texts
            assert re.search(pattern, texts[0]), (pattern, texts[0])
            for e in (eh, ed):          # ... and gone afterwards, the map with it
                with pytest.raises(DavidsonHipError, match="operator not set"):
                    e.apply(OP_A, PANEL_V, 0, 1, PANEL_W, 0)
                with pytest.raises(DavidsonHipError, match="operator not set"):
                    e.update_operator_values(OP_A, data)
        # device-only: the bit widths; null arrays
        assert refusal(ed, True, indptr, indices, data, raw=(0, 16, 64)) == "row_ptr_bits must be 32 or 64"
        assert refusal(ed, True, indptr, indices, data, raw=(0, 64, 8)) == "col_bits must be 32 or 64"
        assert eh.lib.davh_set_operator_csr(eh.h, OP_A, None, None, None, 0, 0) != 0
        assert eh.lib.dav_last_error().decode() == "davh_set_operator_csr: null row_ptr"
        assert ed.lib.davh_set_operator_csr_dev(ed.h, OP_A, None, 64, None, 64, None, 0, 0) != 0
        assert ed.lib.dav_last_error().decode() == "davh_set_operator_csr_dev: null row_ptr"
        rp_d = torch.tensor(indptr, device=DEV)
        assert ed.lib.davh_set_operator_csr_dev(ed.h, OP_A, rp_d.data_ptr(), 64, None, 64, None, 0, 0) != 0
        dev_text = ed.lib.dav_last_error().decode().split(": ", 1)[1]
        assert eh.lib.davh_set_operator_csr(eh.h, OP_A, indptr.ctypes.data, None, None, 0, 0) != 0
        assert eh.lib.dav_last_error().decode().split(": ", 1)[1] == dev_text == "null col_idx or vals"
        # ... and the next set call works, on both
        with fd.CEngine(n=2 * nc, max_cols=COLS) as eb:
            eb.set_operator_bsr(OP_A, indptr, indices, H.expand_blocks(data))
            ref, _ = observe(eb, x)
        eh.set_operator_csr_hermitian(OP_A, indptr, indices, data)
        ed.set_operator_csr_hermitian_dev(OP_A, *to_dev(indptr, indices, data))
        assert_same(observe(eh, x)[0], ref, "host after refusals")
        assert_same(observe(ed, x)[0], ref, "device after refusals")
    # an engine of odd order
    with fd.CEngine(n=2 * nc + 1, max_cols=16) as e:
        texts = [refusal(e, device, indptr, indices, data) for device in (False, True)]
        assert texts[0] == texts[1] and texts[0].startswith(f"n = {2 * nc + 1} is odd"), texts


# ---- T4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lower", [False, True])
def test_refresh_gives_the_bits_of_a_fresh_set_call(lower):
    for nc, kind in ((300, "duplicates"), (1025, "arrowhead"), (17, "missing_diagonal")):
        indptr, indices, data = H.hermitian_csr(nc, kind, lower)
        rows = np.repeat(np.arange(nc), np.diff(indptr))
        rng = np.random.default_rng(9)
        new = data * 1.25          # full input stays Hermitian: the terms of (j, i) are the conjugates of those of (i, j)
        if lower:                  # a lower triangle is free in its strict lower part
            new = data * rng.uniform(0.5, 1.5, data.size) + np.where(rows == indices, 0.0, 1j * rng.uniform(-1e-3, 1e-3, data.size))
        x = rng.standard_normal((2 * nc, COLS))
        dev = to_dev(indptr, indices, data)
        with fd.CEngine(n=2 * nc, max_cols=COLS) as fresh:
            fresh.set_operator_csr_hermitian(OP_A, indptr, indices, new, lower=lower)
            ref, _ = observe(fresh, x)
        for set_dev, upd_dev in itertools.product((False, True), repeat=2):
            with fd.CEngine(n=2 * nc, max_cols=COLS) as e:
                e.keep_value_map(OP_A)
                if set_dev:
                    e.set_operator_csr_hermitian_dev(OP_A, *dev, lower=lower)
                else:
                    e.set_operator_csr_hermitian(OP_A, indptr, indices, data, lower=lower)
                with pytest.raises(TypeError, match="complex128"):
                    e.update_operator_values(OP_A, new.real.copy())
                with pytest.raises(ValueError, match="the set call saw"):
                    e.update_operator_values(OP_A, new[:-1])
                e.update_operator_values(OP_A, torch.tensor(new, device=DEV) if upd_dev else new)
                assert_same(observe(e, x)[0], ref, (nc, kind, set_dev, upd_dev))
                # an imaginary diagonal is refused before a value moves
                dp = np.flatnonzero(rows == indices)
                if dp.size:
                    bad = new.copy()
                    bad[dp[0]] += 1j
                    with pytest.raises(DavidsonHipError, match=rf"diagonal entry {dp[0]} \(row {rows[dp[0]]}\) has the imaginary part 1: the "):
                        e.update_operator_values(OP_A, torch.tensor(bad, device=DEV) if upd_dev else bad)
                    assert_same(observe(e, x)[0], ref, (nc, kind, "after the refused update"))


def test_davidson_engine_refreshes_complex_values(solve_inputs):
    """DavidsonEngine.set_hermitian(keep_map=True) and update_values with host and with device data: the solve of the new values has
    the bits of a fresh engine's; a diagonal with an imaginary part is an exception - never the end of the process - and the operator
    keeps its values"""
    inp = solve_inputs["graded"]
    rp, ci, vv = inp["a"]
    new = vv * 1.5
    nc = inp["h"].shape[0]
    with fd.DavidsonEngine(2 * nc, 2 * LOWEST) as fresh:
        fresh.set_hermitian(1, (rp, ci, new))
        want = fresh.solve("DPR", 400, TOL)
    bad = new.copy()
    dp = np.flatnonzero(ci == np.repeat(np.arange(nc), np.diff(rp)))
    bad[dp[5]] += 2j
    for set_dev, upd_dev in itertools.product((False, True), repeat=2):
        with fd.DavidsonEngine(2 * nc, 2 * LOWEST) as eng:
            a = torch.sparse_csr_tensor(torch.tensor(rp), torch.tensor(ci), torch.tensor(vv), size=(nc, nc)).to(DEV) if set_dev else (rp, ci, vv)
            eng.set_hermitian(1, a, keep_map=True)
            with pytest.raises(TypeError, match="complex128"):
                eng.update_values(1, new.real.copy())
            # host data is checked in Python, device data by the engine: both name the entry and its row from 0
            with pytest.raises(DavidsonHipError if upd_dev else ValueError, match=rf"diagonal entry {dp[5]} .*imaginary part 2"):
                eng.update_values(1, torch.tensor(bad, device=DEV) if upd_dev else bad)
            eng.update_values(1, torch.tensor(new, device=DEV) if upd_dev else new)
            got = eng.solve("DPR", 400, TOL)
            assert got[2] == want[2] and same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (set_dev, upd_dev)


def test_refresh_of_a_real_bsr_operator_on_the_same_engine_is_unchanged():
    nc = 300
    indptr, indices, data = H.hermitian_csr(nc, "random", True)
    blocks = H.expand_blocks(data)
    new_blocks = np.ascontiguousarray(blocks * 0.75)
    x = np.random.default_rng(10).standard_normal((2 * nc, COLS))
    with fd.CEngine(n=2 * nc, max_cols=COLS) as fresh:
        fresh.set_operator_bsr(OP_A, indptr, indices, new_blocks, lower=True)
        ref, _ = observe(fresh, x)
    with fd.CEngine(n=2 * nc, max_cols=COLS) as e:
        e.keep_value_map(OP_A)
        e.set_operator_csr_hermitian(OP_A, indptr, indices, data, lower=True)
        e.update_operator_values(OP_A, data * 0.5)
        e.set_operator_bsr(OP_A, indptr, indices, blocks, lower=True)          # the same slot, now a real BSR operator
        with pytest.raises(TypeError, match="float64"):
            e.update_operator_values(OP_A, data)
        e.update_operator_values(OP_A, new_blocks)
        assert_same(observe(e, x)[0], ref, "host blocks")
        e.update_operator_values(OP_A, torch.tensor(blocks, device=DEV))
        e.update_operator_values(OP_A, torch.tensor(new_blocks, device=DEV))
        assert_same(observe(e, x)[0], ref, "device blocks")


# ---- T5 ------------------------------------------------------------------------------------------------------------------------------
NC, LOWEST, TOL = 200, 4, 1e-8
MATRICES = ("graded", "pencil", "double", "lattice")


@pytest.fixture(scope="module")
def solve_inputs():
    """per matrix: H, S, the CSR arrays of both, eigh's eigenvalues - computed once and left unchanged"""
    sl = pytest.importorskip("scipy.linalg")
    out = {}
    for name in MATRICES:
        h, s = H.solve_matrix(name, NC)
        out[name] = {"h": h, "s": s, "a": H.dense_csr(h), "b": None if s is None else H.dense_csr(s),
                     "ref": sl.eigh(h, s, eigvals_only=True)}
    return out


def check_solution(inp, lam, x, theta, v):
    """eigenvalues against eigh to 1e-8; the residual and orthonormality assertions of the extraction on the engine's real-form pairs"""
    assert np.abs(lam - inp["ref"][:LOWEST]).max() <= 1e-8, (lam, inp["ref"][:LOWEST])
    H.check_extraction(inp["h"], inp["s"], theta, v, lam, x, inp["ref"], tol_lambda=1e-8)


def engine_solve(inp, method, device=False, lower=False, bsr=False):
    """(theta, V, iters) of the real-form solve on a DavidsonEngine; bsr: the operators through set_block_sparse on the expanded blocks"""
    gev, nc = inp["s"] is not None, inp["h"].shape[0]
    with fd.DavidsonEngine(2 * nc, 2 * LOWEST, gev=gev) as eng:
        for which, m, dense in ((1, inp["a"], inp["h"]), (2, inp["b"], inp["s"])):
            if m is None:
                continue
            if lower:
                m = H.dense_csr(dense, lower=True)
            if bsr:
                eng.set_block_sparse(which, m[0], m[1], H.expand_blocks(m[2]), lower=lower)
            elif device:
                eng.set_hermitian(which, torch.sparse_csr_tensor(torch.tensor(m[0]), torch.tensor(m[1]), torch.tensor(m[2]),
                                                                 size=(nc, nc)).to(DEV), lower=lower)
            else:
                eng.set_hermitian(which, m, lower=lower)
        return eng.solve(method, 400, TOL)


@pytest.mark.parametrize("method", ["DPR", "GJD"])
@pytest.mark.parametrize("name", MATRICES)
def test_solves_through_every_front_end(solve_inputs, name, method):
    inp = solve_inputs[name]
    # the engine's real-form pairs, host and device input, and the extraction on them
    theta, v, it = engine_solve(inp, method)
    lam, x = fd.hermitian_eigenpairs(theta, v, LOWEST, inp["b"])
    print(f"{name} {method}: {it} iterations, pair split {np.abs(theta[0::2] - theta[1::2]).max():.3g}")
    assert 0 < it < 400
    check_solution(inp, lam, x, theta, v)
    theta_d, v_d, it_d = engine_solve(inp, method, device=True)
    assert same_bits(theta_d, theta) and same_bits(v_d, v) and it_d == it
    # the bits of the BSR engine on the expanded blocks
    theta_b, v_b, it_b = engine_solve(inp, method, bsr=True)
    assert same_bits(theta_b, theta) and same_bits(v_b, v) and it_b == it
    # the one-shot, from arrays and from a tensor on the GPU
    lam1, x1, it1 = fd.generalized_eigensolver_hermitian(*inp["a"], LOWEST, method, 400, TOL, second=inp["b"])
    assert it1 == it and same_bits(lam1, lam) and same_bits(x1, x)
    t = torch.sparse_csr_tensor(*(torch.tensor(p) for p in inp["a"]), size=inp["h"].shape).to(DEV)
    lam2, x2, it2 = fd.generalized_eigensolver_hermitian(t, None, None, LOWEST, method, 400, TOL, second=inp["b"])
    assert it2 == it and same_bits(lam2, lam) and same_bits(x2, x)


def test_lower_triangle_input_and_a_complex_guess(solve_inputs):
    inp = solve_inputs["pencil"]
    theta, v, it = engine_solve(inp, "DPR", lower=True)
    lam, x = fd.hermitian_eigenpairs(theta, v, LOWEST, H.dense_csr(inp["s"], lower=True), lower=True)
    check_solution(inp, lam, x, theta, v)
    # a warm start from the converged complex vectors: fewer iterations, the same eigenvalues
    lam_w, x_w, it_w = fd.generalized_eigensolver_hermitian(*inp["a"], LOWEST, "DPR", 400, TOL, second=inp["b"], initial_vectors=x)
    assert it_w < it and np.abs(lam_w - inp["ref"][:LOWEST]).max() <= 1e-8


@pytest.mark.parametrize("method", ["CHEB", "LCHEB"])
def test_chebyshev_corrections_on_the_lattice(solve_inputs, method):
    inp = solve_inputs["lattice"]
    theta, v, it = engine_solve(inp, method)
    lam, x = fd.hermitian_eigenpairs(theta, v, LOWEST)
    assert 0 < it < 400
    check_solution(inp, lam, x, theta, v)


def test_bdpr_gives_the_bits_of_dpr(solve_inputs):
    """the diagonal blocks of the real form are d I, so the block-diagonal correction divides by the same numbers as DPR"""
    inp = solve_inputs["graded"]
    theta, v, it = engine_solve(inp, "DPR")
    theta_b, v_b, it_b = engine_solve(inp, "BDPR")
    assert it_b == it and same_bits(theta_b, theta) and same_bits(v_b, v)
