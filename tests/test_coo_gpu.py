"""CSR operators from COO triples (davx_set_operator_coo, davx_set_operator_coo_dev; kernels in fortran_davidson_amd/csrc/k_coo_build.hip).
The triples come in any order, duplicates included; their ROW FORM is the CSR matrix of a stable sort by row (coo_to_csr of
test_sparse_gpu.py), and both entries build bit for bit what dav_set_operator_csr builds from the row form: diagonal, applies and solves
are compared as uint64 bits - over the six matrix classes, full and lower, both bases, the index widths, three orders of the triples; the
order of duplicates; rows at the edges of the sorts; three ranks; the in-register sort against the LDS sort; the value map; storage by
diagonals; every refusal; the front ends; slots B and M."""
import ctypes as C
import itertools
import re
import threading

import numpy as np
import pytest
import torch

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import METHOD_BDPR, OP_A, OP_M, PANEL_V, PANEL_W, DavidsonHipError
from test_sparse_gpu import coo_to_csr, sparse_dd, symmetric_coo

pytestmark = pytest.mark.gpu

CLASSES = ("banded", "random", "empty_rows", "missing_diagonal", "duplicates", "arrowhead")
ORDERS = ("as_generated", "permuted", "reversed")
DEV = "cuda:0"
WIDTHS = {"32/32": (torch.int32, torch.int32), "64/64": (torch.int64, torch.int64), "64/32": (torch.int64, torch.int32)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def triples(n, kind, lower, order, seed=None):
    """(rows, cols, vals) int64 / int64 / float64 of class `kind` in the given order; lower: only the entries with column <= row"""
    rng = np.random.default_rng(CLASSES.index(kind) * 10 + lower if seed is None else seed)
    rows, cols, vals = symmetric_coo(n, kind, rng)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if lower:
        sel = cols <= rows
        rows, cols, vals = rows[sel], cols[sel], vals[sel]
    if order == "permuted":
        p = np.random.default_rng(1234).permutation(rows.size)
        rows, cols, vals = rows[p], cols[p], vals[p]
    elif order == "reversed":
        rows, cols, vals = rows[::-1].copy(), cols[::-1].copy(), vals[::-1].copy()
    return rows, cols, np.ascontiguousarray(vals, dtype=np.float64)


def to_dev(rows, cols, vals, base=0, rt=torch.int64, ct=torch.int64):
    return (torch.tensor(rows + base, dtype=rt, device=DEV), torch.tensor(cols + base, dtype=ct, device=DEV),
            torch.tensor(vals, dtype=torch.float64, device=DEV))


def put_apply_get(e, x, k, which=OP_A):
    e.panel_put(PANEL_V, 0, x[:, :k])
    e.apply(which, PANEL_V, 0, k, PANEL_W, 0)
    return e.panel_get(PANEL_W, 0, k)


def observe(n, put, x, ks=(16, 64), solve=True):
    """what the tests compare of an operator that put(CEngine) sets: the diagonal, the applies at ks columns, a DPR solve"""
    with fd.CEngine(n=n, max_cols=64) as e:
        put(e)
        out = [e.get_diagonal(OP_A)] + [put_apply_get(e, x, k) for k in ks]
    if solve:
        with fd.DavidsonEngine(n, 3) as eng:
            put(eng.c)
            lam, _, it = eng.solve("DPR", 60, 1e-8, want_vectors=False)
        out += [lam, np.array([float(it)])]
    return out


def assert_same(got, ref, what):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and np.array_equal(bits(g), bits(r)), (what, k)


# ---- 1. bitwise equality with the CSR host entry on the row form --------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("kind", CLASSES)
def test_coo_entries_equal_the_csr_host_entry_on_the_row_form(kind, lower, order):
    n = 20011 if kind == "arrowhead" else 1003          # the arrowhead row of 20011 entries takes the tile / merge path
    rows, cols, vals = triples(n, kind, lower, order)
    rp, ci, vv = coo_to_csr(n, rows, cols, vals)
    x = np.random.default_rng(5).standard_normal((n, 64))
    ref = observe(n, lambda e: e.set_operator_csr(OP_A, rp, ci, vv, lower=lower), x)
    for base in (0, 1):
        got = observe(n, lambda e: e.set_operator_coo(OP_A, rows + base, cols + base, vals, base=base, lower=lower), x)
        assert_same(got, ref, ("host", base))
    for (name, (rt, ct)), base in itertools.product(WIDTHS.items(), (0, 1)):
        dev = to_dev(rows, cols, vals, base, rt, ct)
        got = observe(n, lambda e: e.set_operator_coo_dev(OP_A, *dev, base=base, lower=lower), x)
        assert_same(got, ref, ("device", name, base))


# ---- 2. the order of duplicates is the order of the triples ---------------------------------------------------------------------------
@pytest.mark.parametrize("perm", list(itertools.permutations(range(3))))
def test_duplicates_are_summed_in_input_order(perm):
    n = 8
    terms = np.array([1.0, 2.0 ** -60, -1.0])[list(perm)]
    want = ((0.0 + terms[0]) + terms[1]) + terms[2]          # left to right: 0 or 2^-60, by the order
    # the diagonal position (3, 3) and the positions (3, 0) / (0, 3) carry the three terms, the plain diagonal of the other rows in between.
    # The product (k_spmm.hip) deals the canonical entries of a row to four streams in turn and adds the stream sums in stream order: the
    # three terms at column 0 are entries 0, 1, 2 of row 3, one per stream, so the product of row 3 with the unit vector e_0 is their sum
    # from left to right (everything else in the row meets a zero of the vector).
    rows, cols, vals = [], [], []
    others = [i for i in range(n) if i != 3]
    for t in range(3):
        for r, c, v in ((3, 3, terms[t]), (3, 0, terms[t]), (0, 3, terms[t]), (others[2 * t], others[2 * t], 9.0),
                        (others[2 * t + 1], others[2 * t + 1], 9.0)):
            rows.append(r); cols.append(c); vals.append(v)
    rows.append(others[6]); cols.append(others[6]); vals.append(9.0)
    rows, cols, vals = np.array(rows), np.array(cols), np.array(vals)
    unit = np.zeros((n, 1))
    unit[0, 0] = 1.0
    for device in (False, True):
        with fd.CEngine(n=n, max_cols=16) as e:
            if device:
                e.set_operator_coo_dev(OP_A, *to_dev(rows, cols, vals))
            else:
                e.set_operator_coo(OP_A, rows, cols, vals)
            assert bits(e.get_diagonal(OP_A))[3] == bits(np.array([want]))[0], (device, perm)
            y = put_apply_get(e, unit, 1)
            assert bits(y)[3, 0] == bits(np.array([want]))[0], (device, perm, y[3, 0], want)


# ---- 3. row lengths at the edges of the sorts -----------------------------------------------------------------------------------------
def test_row_lengths_at_the_edges_of_the_sorts():
    """lower form: rows 63, 64, 65, 2048, 2049 and 4097 hold that many distinct columns (the in-register sort takes at most 64, one LDS
    tile 2048, 4097 is two tiles and one entry), rows 100 and 101 none, every other row its diagonal entry - all in a random order"""
    n = 4200
    rng = np.random.default_rng(3)
    special = (63, 64, 65, 2048, 2049, 4097)
    rows, cols = [], []
    for i in range(n):
        if i in (100, 101):
            continue
        c = rng.choice(i + 1, size=i, replace=False) if i in special else np.array([i])
        rows.append(np.full(c.size, i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.uniform(-1.0, 1.0, rows.size) + np.where(rows == cols, 10.0, 0.0)
    p = rng.permutation(rows.size)
    rows, cols, vals = rows[p], cols[p], vals[p]
    assert [int((rows == i).sum()) for i in special] == list(special)
    x = rng.standard_normal((n, 64))
    ref = observe(n, lambda e: e.set_operator_csr(OP_A, *coo_to_csr(n, rows, cols, vals), lower=True), x, solve=False)
    assert_same(observe(n, lambda e: e.set_operator_coo(OP_A, rows, cols, vals, lower=True), x, solve=False), ref, "host")
    dev = to_dev(rows, cols, vals, 0, torch.int32, torch.int32)
    assert_same(observe(n, lambda e: e.set_operator_coo_dev(OP_A, *dev, lower=True), x, solve=False), ref, "device")


def test_the_smallest_inputs():
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
    three = (np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), np.array([1.0, -1.0, 2.0 ** -60]))
    for (rows, cols, vals), diag in ((empty, 0.0), (three, 2.0 ** -60)):
        for device in (False, True):
            with fd.CEngine(n=1, max_cols=16) as e:
                if device:
                    e.set_operator_coo_dev(OP_A, *to_dev(rows, cols, vals))
                else:
                    e.set_operator_coo(OP_A, rows, cols, vals)
                assert bits(e.get_diagonal(OP_A))[0] == bits(np.array([diag]))[0]
                assert put_apply_get(e, np.ones((1, 1)), 1)[0, 0] == diag
    # all triples in the last row
    n = 300
    rng = np.random.default_rng(8)
    cols = rng.permutation(n)[:200]
    rows, vals = np.full(cols.size, n - 1), rng.standard_normal(cols.size)
    x = rng.standard_normal((n, 16))
    ref = observe(n, lambda e: e.set_operator_csr(OP_A, *coo_to_csr(n, rows, cols, vals), lower=True), x, ks=(16,), solve=False)
    assert_same(observe(n, lambda e: e.set_operator_coo(OP_A, rows, cols, vals, lower=True), x, ks=(16,), solve=False), ref, "host")
    dev = to_dev(rows, cols, vals)
    assert_same(observe(n, lambda e: e.set_operator_coo_dev(OP_A, *dev, lower=True), x, ks=(16,), solve=False), ref, "device")


def mixed_triples(n, lower, seed):
    """short rows that repeat columns next to rows of more than 64 entries: class `duplicates` (every 5th entry in two terms), rows 0 and
    500 filled to 300 entries with repeated columns among them, and row 700 with 150 terms at its diagonal position - permuted"""
    rng = np.random.default_rng(seed)
    rows, cols, vals = (np.asarray(a) for a in symmetric_coo(n, "duplicates", rng))
    extra_r, extra_c, extra_v = [], [], []
    for i in (0, 500):
        c = rng.integers(0, n, 300)          # with replacement: repeated columns in a long row
        c = c[c != i]
        w = rng.uniform(-1e-3, 1e-3, c.size)
        extra_r += [np.full(c.size, i), c]; extra_c += [c, np.full(c.size, i)]; extra_v += [w, w]
    extra_r.append(np.full(150, 700)); extra_c.append(np.full(150, 700)); extra_v.append(rng.uniform(-1.0, 1.0, 150) * 2.0 ** rng.integers(-40, 1, 150))
    rows = np.concatenate([rows] + extra_r).astype(np.int64)
    cols = np.concatenate([cols] + extra_c).astype(np.int64)
    vals = np.concatenate([vals] + extra_v)
    if lower:
        sel = cols <= rows
        rows, cols, vals = rows[sel], cols[sel], vals[sel]
    p = rng.permutation(rows.size)
    return rows[p], cols[p], np.ascontiguousarray(vals[p])


@pytest.mark.parametrize("keep_map", [False, True])
@pytest.mark.parametrize("lower", [False, True])
def test_duplicates_in_short_rows_next_to_long_rows(lower, keep_map):
    """Once a row exceeds 64 entries the flag pass and the LDS sort run over the arrays that the in-register sort has already ordered: the
    short rows must reach them in key order, ties included, or their duplicates are sorted again by the slot order of the scatter.  The
    diagonal pattern meets the same passes through row 700 (150 terms at one position).  Several seeds: the slot order is not ours to set."""
    n = 1003
    x = np.random.default_rng(12).standard_normal((n, 64))
    for seed in (21, 22, 23):
        rows, cols, vals = mixed_triples(n, lower, seed)
        counts = np.bincount(rows, minlength=n)
        assert counts.max() > 64 and (counts <= 64).sum() > 900
        new = vals * np.random.default_rng(seed).uniform(0.5, 1.5, vals.size)
        ref = observe(n, lambda e: e.set_operator_csr(OP_A, *coo_to_csr(n, rows, cols, vals), lower=lower), x, solve=False)
        ref_new = observe(n, lambda e: e.set_operator_csr(OP_A, *coo_to_csr(n, rows, cols, new), lower=lower), x, solve=False)
        dev = to_dev(rows, cols, vals, 0, torch.int32, torch.int64)
        for device in (False, True):
            with fd.CEngine(n=n, max_cols=64) as e:
                e.keep_value_map(OP_A, keep_map)
                if device:
                    e.set_operator_coo_dev(OP_A, *dev, lower=lower)
                else:
                    e.set_operator_coo(OP_A, rows, cols, vals, lower=lower)
                assert_same([e.get_diagonal(OP_A), put_apply_get(e, x, 16), put_apply_get(e, x, 64)], ref, (seed, device))
                if keep_map:
                    e.update_operator_values(OP_A, torch.tensor(new, device=DEV) if device else new)
                    assert_same([e.get_diagonal(OP_A), put_apply_get(e, x, 16), put_apply_get(e, x, 64)], ref_new, (seed, device, "update"))


# ---- 4. three ranks equal one rank ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "arrowhead"])
def test_three_ranks_equal_one_rank(kind):
    n, nranks = 2999, 3
    rows, cols, vals = triples(n, kind, True, "permuted", seed=17)
    x = np.random.default_rng(17).standard_normal((n, 64))
    with fd.CEngine(n=n, max_cols=64) as e:
        e.set_operator_coo_dev(OP_A, *to_dev(rows, cols, vals, 0, torch.int64, torch.int32), lower=True)
        y1 = put_apply_get(e, x, 64)
    engs = [fd.CEngine(n=n, max_cols=64, rank=r, nranks=nranks) for r in range(nranks)]
    copies = [to_dev(rows, cols, vals, 0, torch.int64, torch.int32) for _ in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def work(r):
        try:
            engs[r].set_operator_coo_dev(OP_A, *copies[r], lower=True)
            out[r] = put_apply_get(engs[r], x, 64)
        except Exception as exc:      # noqa: BLE001
            err[r] = exc
        finally:
            fd.hip_lib().dav_local_group_yield(engs[r].h)

    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join() for t in th]
    row0 = [engs[r].local_rows() for r in range(nranks)]
    for e in engs:
        e.close()
    assert all(x is None for x in err), err
    for r, (r0, nl) in enumerate(row0):
        assert np.array_equal(bits(out[r][r0:r0 + nl]), bits(y1[r0:r0 + nl])), r


# ---- 5. the in-register sort against the LDS sort --------------------------------------------------------------------------------------
def test_the_small_row_sort_equals_the_lds_sort():
    """class random, n = 1003: every row holds at most 64 entries, so the COO entry sorts all of them in registers; the CSR device entry
    on the row form with shuffled rows sorts the same rows in LDS"""
    n = 1003
    rows, cols, vals = triples(n, "random", False, "permuted")
    assert 2 <= np.bincount(rows, minlength=n).max() <= 64
    rp, ci, vv = coo_to_csr(n, rows, cols, vals)             # the row form of the permuted triples: every row in a random order
    assert (np.diff(ci.astype(np.int64)) < 0)[np.setdiff1d(np.arange(ci.size - 1), rp[1:-1] - 1)].sum() > n
    x = np.random.default_rng(9).standard_normal((n, 64))
    csr_dev = (torch.tensor(rp, device=DEV), torch.tensor(ci, device=DEV), torch.tensor(vv, device=DEV))
    ref = observe(n, lambda e: e.set_operator_csr_dev(OP_A, *csr_dev), x, ks=(1, 16, 64), solve=False)
    dev = to_dev(rows, cols, vals)
    assert_same(observe(n, lambda e: e.set_operator_coo_dev(OP_A, *dev), x, ks=(1, 16, 64), solve=False), ref, "small rows")


# ---- 6. the value map -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("kind", ["duplicates", "missing_diagonal"])
def test_updates_take_the_values_in_the_order_of_the_triples(kind, lower):
    n = 1003
    rows, cols, vals = triples(n, kind, lower, "permuted")
    new = vals * np.random.default_rng(2).uniform(0.5, 1.5, vals.size)          # (nothing here reads the symmetry of the new matrix)
    x = np.random.default_rng(6).standard_normal((n, 64))
    fresh = observe(n, lambda e: e.set_operator_coo(OP_A, rows, cols, new, lower=lower), x, ks=(64,), solve=False)
    for set_dev in (False, True):
        for update_dev in (False, True):
            with fd.CEngine(n=n, max_cols=64) as e:
                e.keep_value_map(OP_A)
                if set_dev:
                    e.set_operator_coo_dev(OP_A, *to_dev(rows, cols, vals), lower=lower)
                else:
                    e.set_operator_coo(OP_A, rows, cols, vals, lower=lower)
                e.update_operator_values(OP_A, torch.tensor(new, device=DEV) if update_dev else new)
                assert_same([e.get_diagonal(OP_A), put_apply_get(e, x, 64)], fresh, (set_dev, update_dev))


def test_an_update_without_the_map_is_refused():
    n = 300
    rows, cols, vals = sparse_dd(n, 5)
    with fd.CEngine(n=n, max_cols=16) as e:
        for device in (False, True):
            if device:
                e.set_operator_coo_dev(OP_A, *to_dev(rows, cols, vals))
            else:
                e.set_operator_coo(OP_A, rows, cols, vals)
            with pytest.raises(DavidsonHipError, match="dav_keep_value_map"):
                e.update_operator_values(OP_A, vals)


# ---- 7. DAV_CSR_DIAGONALS -------------------------------------------------------------------------------------------------------------
def test_storage_by_diagonals_from_triples():
    n = 1003
    rows, cols, vals = triples(n, "banded", False, "permuted")
    rp, ci, vv = coo_to_csr(n, rows, cols, vals)
    x = np.random.default_rng(7).standard_normal((n, 64))
    ref = observe(n, lambda e: e.set_operator_csr(OP_A, rp, ci, vv, diagonals=True), x)
    assert_same(observe(n, lambda e: e.set_operator_coo(OP_A, rows, cols, vals, diagonals=True), x), ref, "host")
    dev = to_dev(rows, cols, vals)
    assert_same(observe(n, lambda e: e.set_operator_coo_dev(OP_A, *dev, diagonals=True), x), ref, "device")
    # the kind is DIA: BDPR says what the operator is
    m = 4
    for device in (False, True):
        with fd.CEngine(n=n, max_cols=16) as e:
            if device:
                e.set_operator_coo_dev(OP_A, *dev, diagonals=True)
            else:
                e.set_operator_coo(OP_A, rows, cols, vals, diagonals=True)
            e.panel_put(PANEL_V, 0, x[:, :m])
            e.panel_put(PANEL_W, 0, x[:, m:2 * m])
            with pytest.raises(DavidsonHipError, match=re.escape("operator A is a CSR matrix stored by diagonals")):
                e.ritz_residual_correction(m, 1, np.eye(m), np.arange(m, dtype=np.float64), METHOD_BDPR)
    # class random: refused with the message of the CSR entry on the row form, the operator left unset
    rows, cols, vals = triples(n, "random", False, "permuted")
    with fd.CEngine(n=n, max_cols=16) as e:
        with pytest.raises(DavidsonHipError) as want:
            e.set_operator_csr(OP_A, *coo_to_csr(n, rows, cols, vals), diagonals=True)
        for device in (False, True):
            with pytest.raises(DavidsonHipError) as got:
                if device:
                    e.set_operator_coo_dev(OP_A, *to_dev(rows, cols, vals), diagonals=True)
                else:
                    e.set_operator_coo(OP_A, rows, cols, vals, diagonals=True)
            assert _suffix(str(got.value)) == _suffix(str(want.value)) and "DIA_MAX_FILL" in str(got.value)
            with pytest.raises(DavidsonHipError, match="operator not set"):
                e.apply(OP_A, PANEL_V, 0, 1, PANEL_W, 0)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def _suffix(msg):
    return re.sub(r"^davx?_set_operator_(csr|coo)(_dev)?: ", "", msg)


def test_refusals_name_the_first_triple_and_leave_the_engine_usable():
    n = 500
    rows, cols, vals = (np.asarray(a) for a in sparse_dd(n, 51))
    rows, cols = rows.astype(np.int64), cols.astype(np.int64)
    p = np.random.default_rng(0).permutation(rows.size)
    rows, cols, vals = rows[p], cols[p], vals[p]

    def changed(which, at, to):
        r, c = rows.copy(), cols.copy()
        (r if which == "row" else c)[list(at)] = to
        return r, c

    above = int(np.argmax(cols > rows))
    two = changed("col", (1500, 40), [n + 3, -7])          # two offending triples: the one at the smaller p is named
    one_based = (np.where(np.arange(rows.size) == 5, 0, rows + 1), cols + 1)
    cases = [(changed("row", (17,), [-1]), {}, "row index -1 out of range at entry 17"),
             (changed("row", (17,), [n]), {}, f"row index {n} out of range at entry 17"),
             (one_based, {"base": 1}, "row index 0 out of range at entry 6"),
             (changed("col", (29,), [n]), {}, f"column index {n} out of range at entry 29 (row {rows[29]})"),
             ((rows, cols), {"lower": True}, f"entry ({rows[above]}, {cols[above]}) lies above the diagonal of a DAV_CSR_LOWER matrix"),
             (two, {}, f"column index -7 out of range at entry 40 (row {rows[40]})")]
    lib = fd.hip_lib()
    with fd.CEngine(n=n, max_cols=16) as e:
        def unset():
            with pytest.raises(DavidsonHipError, match="operator not set"):
                e.apply(OP_A, PANEL_V, 0, 1, PANEL_W, 0)
        for (r, c), kw, text in cases:
            with pytest.raises(DavidsonHipError) as host:
                e.set_operator_coo(OP_A, r, c, vals, **kw)
            assert _suffix(str(host.value)) == text
            unset()
            for rt, ct in WIDTHS.values():
                dev = (torch.tensor(r, dtype=rt, device=DEV), torch.tensor(c, dtype=ct, device=DEV), torch.tensor(vals, device=DEV))
                with pytest.raises(DavidsonHipError) as got:
                    e.set_operator_coo_dev(OP_A, *dev, **kw)
                assert _suffix(str(got.value)) == _suffix(str(host.value))
                unset()
        # arguments the front ends cannot produce: straight to the C entries
        r32, c32 = rows.astype(np.int32), cols.astype(np.int32)
        d_r, d_c, d_v = torch.tensor(r32, device=DEV), torch.tensor(c32, device=DEV), torch.tensor(vals, device=DEV)
        ptr = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
        hp = lambda a: C.c_void_p(a.ctypes.data)     # noqa: E731
        nnz = rows.size
        for host_args, dev_args, msg in (
                ((-1, hp(r32), hp(c32), hp(vals), 0, 0), (-1, ptr(d_r), 32, ptr(d_c), 32, ptr(d_v), 0, 0), "nnz = -1 must not be negative"),
                ((nnz, hp(r32), hp(c32), None, 0, 0), (nnz, ptr(d_r), 32, ptr(d_c), 32, None, 0, 0), "null vals"),
                ((nnz, hp(r32), hp(c32), hp(vals), 2, 0), (nnz, ptr(d_r), 32, ptr(d_c), 32, ptr(d_v), 2, 0), "index_base must be 0 or 1"),
                ((nnz, hp(r32), hp(c32), hp(vals), 0, 4), (nnz, ptr(d_r), 32, ptr(d_c), 32, ptr(d_v), 0, 4),
                 "triangle must be DAV_CSR_FULL or DAV_CSR_LOWER")):
            assert lib.davx_set_operator_coo(e.h, OP_A, *host_args) != 0
            assert _suffix(lib.dav_last_error().decode()) == msg
            assert lib.davx_set_operator_coo_dev(e.h, OP_A, *dev_args) != 0
            assert _suffix(lib.dav_last_error().decode()) == msg
            unset()
        for dev_args, msg in (((nnz, ptr(d_r), 16, ptr(d_c), 32, ptr(d_v), 0, 0), "row_bits must be 32 or 64"),
                              ((nnz, ptr(d_r), 32, ptr(d_c), 48, ptr(d_v), 0, 0), "col_bits must be 32 or 64"),
                              ((nnz, hp(r32), 32, ptr(d_c), 32, ptr(d_v), 0, 0), "row_idx is not device memory"),
                              ((nnz, ptr(d_r), 32, hp(c32), 32, ptr(d_v), 0, 0), "col_idx is not device memory")):
            assert lib.davx_set_operator_coo_dev(e.h, OP_A, *dev_args) != 0
            assert _suffix(lib.dav_last_error().decode()).startswith(msg), lib.dav_last_error().decode()
            unset()
        # a device row_idx allocation shorter than nnz: refused before any launch (an allocation of its own, so the runtime knows its end)
        hip = C.CDLL("libamdhip64.so")
        short = C.c_void_p()
        assert hip.hipMalloc(C.byref(short), C.c_size_t(4 * (nnz - 100))) == 0
        try:
            assert lib.davx_set_operator_coo_dev(e.h, OP_A, nnz, short, 32, ptr(d_c), 32, ptr(d_v), 0, 0) != 0
            assert _suffix(lib.dav_last_error().decode()) == f"row_idx holds fewer than the {4 * nnz} bytes the matrix needs"
        finally:
            hip.hipFree(short)
        unset()
        # the engine then takes a valid matrix, through either entry
        x = np.random.default_rng(1).standard_normal((n, 8))
        e.set_operator_coo_dev(OP_A, d_r, d_c, d_v)
        y = put_apply_get(e, x, 8)
        e.set_operator_coo(OP_A, rows, cols, vals)
        assert np.array_equal(bits(y), bits(put_apply_get(e, x, 8)))


# ---- 9. front ends --------------------------------------------------------------------------------------------------------------------
def dup_triples(n, seed, diag=None):
    """sparse_dd with every third triple split into two terms at the same position, in a fixed random order"""
    rows, cols, vals = sparse_dd(n, seed, diag=diag)
    sel = np.arange(rows.size) % 3 == 0
    rows, cols = np.concatenate([rows, rows[sel]]), np.concatenate([cols, cols[sel]])
    vals = np.concatenate([np.where(sel, 0.625 * vals, vals), 0.375 * vals[sel]])
    p = np.random.default_rng(seed).permutation(rows.size)
    return rows[p].astype(np.int64), cols[p].astype(np.int64), vals[p]


def torch_coo(rows, cols, vals, n, device):
    t = torch.sparse_coo_tensor(torch.tensor(np.stack([rows, cols])), torch.tensor(vals), size=(n, n)).to(device)
    assert not t.is_coalesced()
    return t


def same_solve(got, ref):
    assert got[2] == ref[2] and np.array_equal(bits(got[0]), bits(ref[0])), (got[2], ref[2], got[0], ref[0])


def test_front_ends_read_the_triples_as_they_stand():
    n, lowest = 1501, 4
    a, b = dup_triples(n, 61), dup_triples(n, 62, diag=2.0)
    ref = fd.generalized_eigensolver_coo(*a, n, lowest, "DPR", 200, 1e-8)
    ref_g = fd.generalized_eigensolver_coo(*a, n, lowest, "DPR", 200, 1e-8, second=b)
    assert 0 < ref[2] < 200 and 0 < ref_g[2] < 200
    with fd.DavidsonEngine(n, lowest) as eng:          # the row form through the CSR front end: the same operator
        eng.set_sparse(1, *coo_to_csr(n, *a))
        same_solve(eng.solve("DPR", 200, 1e-8, want_vectors=False), ref)
    for device in (DEV, "cpu"):
        ta, tb = torch_coo(*a, n, device), torch_coo(*b, n, device)
        with fd.DavidsonEngine(n, lowest) as eng:
            eng.set_coo(1, ta)
            same_solve(eng.solve("DPR", 200, 1e-8, want_vectors=False), ref)
        with fd.DavidsonEngine(n, lowest, gev=True) as eng:
            eng.set_sparse(1, ta)
            eng.set_sparse(2, tb)
            same_solve(eng.solve("DPR", 200, 1e-8, want_vectors=False), ref_g)
        same_solve(fd.generalized_eigensolver_sparse(ta, None, None, lowest, "DPR", 200, 1e-8), ref)
        same_solve(fd.generalized_eigensolver_sparse(ta, None, None, lowest, "DPR", 200, 1e-8, second=tb), ref_g)
        same_solve(fd.generalized_eigensolver_coo(ta, None, None, None, lowest, "DPR", 200, 1e-8, second=tb), ref_g)
    # three CPU tensors given one by one take the host path, as three numpy arrays do
    same_solve(fd.generalized_eigensolver_coo(*(torch.tensor(v) for v in a), n, lowest, "DPR", 200, 1e-8), ref)
    with fd.CEngine(n=n, max_cols=16) as e:
        e.set_operator_coo(OP_A, *(torch.tensor(v) for v in a))
        d = e.get_diagonal(OP_A)
        e.set_operator_coo(OP_A, *a)
        assert np.array_equal(bits(d), bits(e.get_diagonal(OP_A)))
    # device tensors as three arrays
    same_solve(fd.generalized_eigensolver_coo(*to_dev(*a), n, lowest, "DPR", 200, 1e-8, second=to_dev(*b)), ref_g)


def test_a_scipy_coo_matrix_is_read_without_summing_duplicates():
    sp = pytest.importorskip("scipy.sparse")
    n, lowest = 1501, 4
    a = dup_triples(n, 61)
    ref = fd.generalized_eigensolver_coo(*a, n, lowest, "DPR", 200, 1e-8)
    m = sp.coo_matrix((a[2], (a[0], a[1])), shape=(n, n))
    assert m.nnz == a[2].size
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_coo(1, m)
        same_solve(eng.solve("DPR", 200, 1e-8, want_vectors=False), ref)
    same_solve(fd.generalized_eigensolver_coo(m, None, None, None, lowest, "DPR", 200, 1e-8), ref)


# ---- 10. slots B and M ----------------------------------------------------------------------------------------------------------------
def test_the_preconditioner_as_permuted_triples():
    import precond_inputs as P
    a, b, m, lowest = P.solve_case("n400_gev")
    n = a.shape[0]
    rng = np.random.default_rng(4)

    def as_triples(dense, full=False):
        rp, ci, vv = P.csr_of(dense, full=full)
        rows = np.repeat(np.arange(n), np.diff(rp))
        p = rng.permutation(rows.size)
        return rows[p], ci[p].astype(np.int64), vv[p]

    out = []
    for coo_m in (False, True):
        for device in ((False,) if not coo_m else (False, True)):
            with fd.DavidsonEngine(n, lowest, None, gev=True) as eng:
                ta, tb, tm = as_triples(a), as_triples(b), as_triples(m, full=True)
                eng.set_coo(1, *(to_dev(*ta) if device else ta))
                eng.set_coo(2, *(to_dev(*tb) if device else tb))
                if coo_m:
                    eng.set_coo(3, *(to_dev(*tm) if device else tm))
                else:
                    eng.set_sparse(3, *P.csr_of(m, full=True))
                out.append(eng.solve("DPR", P.MAX_ITERATIONS, P.TOLERANCE, want_vectors=False))
    assert 0 < out[0][2] < P.MAX_ITERATIONS
    same_solve(out[1], out[0])
    same_solve(out[2], out[0])
    with fd.CEngine(n=n, max_cols=16) as e:          # the slot itself: M applied from triples equals M applied from CSR
        x = rng.standard_normal((n, 16))
        e.set_operator_csr(OP_M, *P.csr_of(m, full=True))
        y = put_apply_get(e, x, 16, which=OP_M)
        e.set_operator_coo_dev(OP_M, *to_dev(*as_triples(m, full=True)))
        assert np.array_equal(bits(y), bits(put_apply_get(e, x, 16, which=OP_M)))
