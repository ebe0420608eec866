"""New values on the kept pattern of a sparse operator (dav_keep_value_map, dav_update_operator_values, dav_update_operator_values_dev).
The yardstick is always a FRESH set call with the new values on another engine - the existing entry, not the code under test - and the
comparison is bitwise: the diagonal, a 16- and a 64-column apply, eigenvalues and iteration count of a DPR solve.  Over the six CSR
classes and the BSR block sizes, full and lower storage, both bases and block layouts, sorted and shuffled input, operators set from host
or device arrays and updated from host or device arrays; three ranks; repeated and mixed updates; every refusal; the front ends."""
import ctypes as C
import functools
import itertools
import re
import threading

import numpy as np
import pytest
import torch

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import BSR_ROW_MAJOR, OP_A, OP_B, PANEL_V, PANEL_W, DavidsonHipError
from test_bsr_device_gpu import blocks_of, sorted_bsr_input
from test_bsr_gpu import STORAGES, bsr_input, symmetric_blocks
from test_sparse_device_gpu import CLASSES, bits, put_apply_get, shuffled_rows, sorted_csr
from test_sparse_gpu import coo_to_csr, sparse_dd, symmetric_coo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = 2048                 # entries per workgroup of the CSR gather (k_sparse_refresh.hip)


def new_values(vv):
    """other numbers on the same pattern, a function of the old value alone (so a symmetric matrix stays symmetric and diagonally
    dominant): every entry differs from the old one"""
    out = np.where(np.abs(vv) < 0.5, 1.25 * vv, vv + 3.0 + 0.1 * np.abs(vv))
    assert (out != vv).all()
    return out


def dev(a, dtype=None):
    return torch.tensor(a, dtype=dtype, device=DEV)


def observe(n, put, x, solve=True):
    """(diagonal, 16-column apply, 64-column apply, eigenvalues, iterations) of the operator `put` leaves in an engine"""
    with fd.CEngine(n=n, max_cols=64) as e:
        put(e)
        d = e.get_diagonal(OP_A)
        y16, y64 = put_apply_get(e, x, 16), put_apply_get(e, x, 64)
    lam, it = np.zeros(0), 0
    if solve:
        with fd.DavidsonEngine(n, 4) as eng:
            put(eng.c)
            lam, _, it = eng.solve("DPR", 60, 1e-8, want_vectors=False)
    return d, y16, y64, lam, it


def assert_same(got, ref, what=None):
    (d0, a0, b0, l0, i0), (d1, a1, b1, l1, i1) = got, ref
    assert np.array_equal(bits(d0), bits(d1)), what
    assert np.array_equal(bits(a0), bits(a1)), what
    assert np.array_equal(bits(b0), bits(b1)), what
    assert i0 == i1 and np.array_equal(bits(l0), bits(l1)), (what, i0, i1, l0, l1)


# ---- CSR inputs and their yardsticks -------------------------------------------------------------------------------------------------
def csr_n(kind):
    return 2500 if kind == "arrowhead" else 1050     # arrowhead, lower: row 0 mirrors 2499 entries (> the LDS sort tile, > CSR_CHUNK)


@functools.lru_cache(maxsize=None)
def csr_case(kind, lower, shuffled):
    """(n, rp, ci, old values, new values, x, yardstick): the yardstick is a fresh host set call with the new values, computed once"""
    n = csr_n(kind)
    rng = np.random.default_rng(CLASSES.index(kind) * 10 + lower)
    rows, cols, vals = symmetric_coo(n, kind, rng)
    rp, ci, vv = sorted_csr(n, rows, cols, vals, lower)
    if shuffled:
        rp, ci, vv = shuffled_rows(rp, ci, vv, rng)
    vv2 = new_values(vv)
    x = rng.standard_normal((n, 64))
    ref = observe(n, lambda e: e.set_operator_csr(OP_A, rp, ci, vv2, lower=lower), x)
    for a in (rp, ci, vv, vv2, x, *ref[:4]):
        a.setflags(write=False)
    return n, rp, ci, vv, vv2, x, ref


def csr_set(e, rp, ci, vv, base, lower, device):
    if device:
        e.set_operator_csr_dev(OP_A, dev(rp + base), dev(ci.astype(np.int64) + base, torch.int32), dev(vv), base=base, lower=lower)
    else:
        e.set_operator_csr(OP_A, rp + base, ci + base, vv, base=base, lower=lower)


def update(e, which, vals, device):
    e.update_operator_values(which, dev(vals) if device else vals)


# ---- 1. the map changes nothing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CLASSES)
@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("device", [False, True])
def test_an_operator_built_with_the_map_equals_one_built_without(kind, lower, device):
    """the CSR order step with the source of an entry as payload (and the gather behind it) against the value payload"""
    n, rp, ci, vv, _, x, _ = csr_case(kind, lower, True)
    out = []
    for on in (False, True):
        with fd.CEngine(n=n, max_cols=64) as e:
            e.keep_value_map(OP_A, on)
            csr_set(e, rp, ci, vv, 0, lower, device)
            out.append((e.get_diagonal(OP_A), put_apply_get(e, x, 16), put_apply_get(e, x, 64)))
    for a, b in zip(*out):
        assert np.array_equal(bits(a), bits(b))


# ---- 2. CSR refresh ------------------------------------------------------------------------------------------------------------------
BASE_ORDER = [(0, False), (1, True), (0, True), (1, False)]


def _csr_cases():
    """class x triangle x how the operator was set x how it is updated, each with two of the four (base, order) pairs: 96 cases in
    which every class and triangle meets every base, order, set entry and update entry"""
    for idx, (kind, lower, set_dev, upd_dev) in enumerate(itertools.product(CLASSES, (False, True), (False, True), (False, True))):
        for t in (0, 1):
            base, shuffled = BASE_ORDER[(idx + t) % 4]
            yield kind, lower, base, shuffled, set_dev, upd_dev


@pytest.mark.parametrize("kind,lower,base,shuffled,set_dev,upd_dev", list(_csr_cases()))
def test_csr_update_equals_a_fresh_set(kind, lower, base, shuffled, set_dev, upd_dev):
    n, rp, ci, vv, vv2, x, ref = csr_case(kind, lower, shuffled)

    def put(e):
        e.keep_value_map(OP_A)
        csr_set(e, rp, ci, vv, base, lower, set_dev)
        update(e, OP_A, vv2, upd_dev)

    assert_same(observe(n, put, x), ref, (kind, lower, base, shuffled, set_dev, upd_dev))


def test_the_gather_tail_runs():
    """banded, full: 7338 local entries = 3 whole tiles of the gather and a tail of 1194"""
    _, rp, *_ = csr_case("banded", False, False)
    assert rp[-1] == 3 * TILE + 1194


@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("set_dev,upd_dev", [(False, True), (True, False)])
def test_signed_zeros_on_the_diagonal(lower, set_dev, upd_dev):
    """no NaN anywhere; diagonal entries -0.0, +0.0, pairs x, -x of a split entry and a single -0.0: the sum starts from +0.0 in input
    order, as the set calls form it"""
    n, rp, ci, vv, vv2, x, _ = csr_case("duplicates", lower, True)
    rows = np.repeat(np.arange(n), np.diff(rp))
    vv2 = vv2.copy()
    on = np.flatnonzero(ci == rows)                                   # diagonal entries, in input order
    places = {}
    for p in on:
        places.setdefault(int(rows[p]), []).append(p)
    assert any(len(v) == 2 for v in places.values())                  # the class splits the diagonal entry of every fifth row
    for r, ps in places.items():
        if len(ps) == 2 and r % 10 == 0:
            vv2[ps] = -0.0                                            # +0.0 + -0.0 + -0.0
        elif len(ps) == 2:
            vv2[ps[1]] = -vv2[ps[0]]                                  # +0.0 + x - x
        elif r % 5 == 1:
            vv2[ps] = -0.0
        elif r % 5 == 2:
            vv2[ps] = 0.0
    assert (vv2 != vv).all() and not np.isnan(vv2).any()
    ref = observe(n, lambda e: e.set_operator_csr(OP_A, rp, ci, vv2, lower=lower), x, solve=False)
    assert np.signbit(vv2[on]).any() and (ref[0] == 0).any() and not np.signbit(ref[0][ref[0] == 0]).any()

    def put(e):
        e.keep_value_map(OP_A)
        csr_set(e, rp, ci, vv, 0, lower, set_dev)
        update(e, OP_A, vv2, upd_dev)

    assert_same(observe(n, put, x, solve=False), ref)


# ---- 3. BSR refresh ------------------------------------------------------------------------------------------------------------------
def bsr_n(b):
    return 1050 if b in (3, 5) else 1056


@functools.lru_cache(maxsize=None)
def bsr_case(kind, b, storage, shuffled):
    lower, _, layout = STORAGES[storage]
    n = bsr_n(b)
    nb = n // b
    rng = np.random.default_rng(1000 * len(kind) + 10 * b + storage)
    bi, bj, blk = blocks_of(nb, b, rng, kind)
    if shuffled:
        rp, ci, vv = bsr_input(nb, bi, bj, blk, lower, layout, rng)
    else:
        rp, ci, vv = sorted_bsr_input(nb, bi, bj, blk, lower, layout)
    vv2 = new_values(vv)
    x = rng.standard_normal((n, 64))
    ref = observe(n, lambda e: e.set_operator_bsr(OP_A, rp, ci, vv2, lower=lower, layout=layout), x)
    for a in (rp, ci, vv, vv2, x, *ref[:4]):
        a.setflags(write=False)
    return n, rp, ci, vv, vv2, x, ref


def bsr_set(e, rp, ci, vv, base, lower, layout, device, which=OP_A):
    if device:
        e.set_operator_bsr_dev(which, dev(rp + base), dev(ci.astype(np.int64) + base, torch.int32), dev(vv), base=base, lower=lower,
                               layout=layout)
    else:
        e.set_operator_bsr(which, rp + base, ci + base, vv, base=base, lower=lower, layout=layout)


SET_UPDATE = [(False, False), (True, True), (False, True), (True, False)]


def _bsr_cases():
    """block size x the four storages (triangle, base, layout), each with two of the four (set entry, update entry) pairs: 56 cases;
    then the arrowhead whose first block row holds 350 blocks (3 chunks of the block product) in every storage"""
    for idx, (b, storage) in enumerate(itertools.product((1, 3, 4, 5, 8, 12, 16), range(4))):
        for t in (0, 1):
            set_dev, upd_dev = SET_UPDATE[(idx + t) % 4]
            yield ("random", "split_diagonal")[(idx + t) % 2], b, storage, (idx + t) % 2 == 0, set_dev, upd_dev
    for storage in range(4):
        yield "arrowhead", 3, storage, True, *SET_UPDATE[storage]


@pytest.mark.parametrize("kind,b,storage,shuffled,set_dev,upd_dev", list(_bsr_cases()))
def test_bsr_update_equals_a_fresh_set(kind, b, storage, shuffled, set_dev, upd_dev):
    lower, base, layout = STORAGES[storage]
    n, rp, ci, vv, vv2, x, ref = bsr_case(kind, b, storage, shuffled)
    if kind == "arrowhead":
        assert n // b == 350 and (np.diff(rp)[0] == 350 or lower)

    def put(e):
        e.keep_value_map(OP_A)
        bsr_set(e, rp, ci, vv, base, lower, layout, set_dev)
        update(e, OP_A, vv2 if (b + storage) % 2 else vv2.reshape(-1), upd_dev)       # (nnzb, b, b) or flat

    assert_same(observe(n, put, x), ref, (kind, b, storage, shuffled, set_dev, upd_dev))


# ---- 4. three ranks against one ------------------------------------------------------------------------------------------------------
def three_rank_refresh(n, set_op, vals, upd_dev, x, k=16):
    """set with the map, update and apply k columns on three ranks (every rank with the global arrays, as the set calls take them)"""
    nranks = 3
    engs = [fd.CEngine(n=n, max_cols=64, rank=r, nranks=nranks) for r in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def work(r):
        try:
            engs[r].keep_value_map(OP_A)
            set_op(engs[r])
            update(engs[r], OP_A, vals, upd_dev)
            out[r] = put_apply_get(engs[r], x, k)
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
    assert all(v is None for v in err), err
    return out, row0


@pytest.mark.parametrize("kind,set_dev,upd_dev", [("random", False, True), ("arrowhead", True, False)])
def test_three_ranks_csr_update_equals_one_rank_fresh_set(kind, set_dev, upd_dev):
    n, rp, ci, vv, vv2, x, ref = csr_case(kind, True, True)
    out, row0 = three_rank_refresh(n, lambda e: csr_set(e, rp, ci, vv, 0, True, set_dev), vv2, upd_dev, x)
    for r, (r0, nl) in enumerate(row0):
        assert np.array_equal(bits(out[r][r0:r0 + nl]), bits(ref[1][r0:r0 + nl])), r


@pytest.mark.parametrize("b,set_dev,upd_dev", [(5, True, True), (12, False, False)])
def test_three_ranks_bsr_update_equals_one_rank_fresh_set(b, set_dev, upd_dev):
    """slabs of 352 rows: block rows of b = 5 at N = 1050 and of b = 12 at N = 1056 straddle two ranks"""
    storage = 3                                             # lower, base 0, row-major
    lower, base, layout = STORAGES[storage]
    n, rp, ci, vv, vv2, x, ref = bsr_case("random", b, storage, True)
    out, row0 = three_rank_refresh(n, lambda e: bsr_set(e, rp, ci, vv, base, lower, layout, set_dev), vv2, upd_dev, x)
    assert any(r0 % b for r0, _ in row0)
    for r, (r0, nl) in enumerate(row0):
        assert np.array_equal(bits(out[r][r0:r0 + nl]), bits(ref[1][r0:r0 + nl])), r


# ---- 5. repeat and mix ---------------------------------------------------------------------------------------------------------------
def state(e, x, which=OP_A):
    e.panel_put(PANEL_V, 0, x[:, :16])
    e.apply(which, PANEL_V, 0, 16, PANEL_W, 0)
    return e.get_diagonal(which), e.panel_get(PANEL_W, 0, 16)


def same_state(a, b):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


def test_updates_in_a_row_and_back_reproduce_the_first_bits():
    n, rp, ci, vv, vv2, x, ref = csr_case("duplicates", True, True)
    vv3 = new_values(vv2)
    with fd.CEngine(n=n, max_cols=64) as e:
        e.keep_value_map(OP_A)
        csr_set(e, rp, ci, vv, 0, True, True)
        first = state(e, x)
        update(e, OP_A, vv2, True)
        second = state(e, x)
        update(e, OP_A, vv3, False)
        assert not same_state(state(e, x), second)
        update(e, OP_A, vv2, False)
        assert same_state(state(e, x), second) and same_state(second, (ref[0], ref[1]))
        update(e, OP_A, vv, True)
        assert same_state(state(e, x), first)


def test_two_sparse_operators_are_updated_independently_and_a_set_call_follows():
    n, rp, ci, vv, vv2, x, ref = csr_case("random", False, False)
    lower, base, layout = STORAGES[1]                     # B: a BSR matrix of the same order, b = 5, lower, base 1, column-major
    rng = np.random.default_rng(5)
    nbr = n // 5
    bi, bj, blk = symmetric_blocks(nbr, 5, rng, "random")
    brp, bci, bvv = bsr_input(nbr, bi, bj, blk, lower, layout, rng)
    bvv2 = new_values(bvv)
    with fd.CEngine(n=n, max_cols=64, gev=True) as e, fd.CEngine(n=n, max_cols=64, gev=True) as fresh:
        e.keep_value_map(OP_A)
        e.keep_value_map(OP_B)
        csr_set(e, rp, ci, vv, 0, False, False)
        bsr_set(e, brp, bci, bvv, base, lower, layout, True, which=OP_B)
        a_old, b_old = state(e, x, OP_A), state(e, x, OP_B)
        fresh.set_operator_csr(OP_A, rp, ci, vv2)
        fresh.set_operator_bsr(OP_B, brp + base, bci + base, bvv2, base=base, lower=lower, layout=layout)
        a_new, b_new = state(fresh, x, OP_A), state(fresh, x, OP_B)
        update(e, OP_A, vv2, True)
        assert same_state(state(e, x, OP_A), a_new) and same_state(state(e, x, OP_B), b_old)
        update(e, OP_A, vv, False)
        update(e, OP_B, bvv2, False)
        assert same_state(state(e, x, OP_A), a_old) and same_state(state(e, x, OP_B), b_new)
        # a set call after an update works; with the switch off by then it drops the map
        e.keep_value_map(OP_A, False)
        csr_set(e, rp, ci, vv2, 1, False, True)
        assert same_state(state(e, x, OP_A), a_new)
        with pytest.raises(DavidsonHipError, match="dav_keep_value_map"):
            update(e, OP_A, vv, False)
        assert same_state(state(e, x, OP_A), a_new) and same_state(state(e, x, OP_B), b_new)
        update(e, OP_B, bvv, True)                        # B kept its map
        assert same_state(state(e, x, OP_B), b_old)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def _suffix(msg):
    return re.sub(r"^dav_update_operator_values(_dev)?: ", "", msg)


def test_refusals_leave_the_operator_applying_with_its_old_bits():
    n, rp, ci, vv, vv2, x, _ = csr_case("random", True, True)
    lib = fd.hip_lib()
    with fd.CEngine(n=n, max_cols=64, gev=True) as e:
        # set without the map
        csr_set(e, rp, ci, vv, 0, True, False)
        old = state(e, x)
        for device in (False, True):
            with pytest.raises(DavidsonHipError) as got:
                update(e, OP_A, vv2, device)
            assert _suffix(str(got.value)).startswith("the operator was set without its value map: call dav_keep_value_map")
            assert same_state(state(e, x), old)
        # a slot holding a dense or an identity operator
        e.set_operator_identity(OP_B)
        b_old = state(e, x, OP_B)
        with pytest.raises(DavidsonHipError, match="is not a CSR or BSR operator .*dav_keep_value_map"):
            update(e, OP_B, vv2, False)
        assert same_state(state(e, x, OP_B), b_old)
        e.set_dense_host(OP_B, np.diag(1.0 + np.arange(n)))
        b_old = state(e, x, OP_B)
        with pytest.raises(DavidsonHipError, match="is not a CSR or BSR operator .*dav_keep_value_map"):
            update(e, OP_B, vv2, True)
        assert same_state(state(e, x, OP_B), b_old)
        # with the map: the pointers
        e.keep_value_map(OP_A)
        csr_set(e, rp, ci, vv, 0, True, True)
        assert same_state(state(e, x), old)
        for entry in (lib.dav_update_operator_values, lib.dav_update_operator_values_dev):
            assert entry(e.h, OP_A, None) != 0
            assert _suffix(lib.dav_last_error().decode()) == "null vals"
        assert lib.dav_update_operator_values_dev(e.h, OP_A, C.c_void_p(vv2.ctypes.data)) != 0       # pageable host memory
        assert "vals is not device memory" in lib.dav_last_error().decode()
        hip = C.CDLL("libamdhip64.so")
        pinned = C.c_void_p()
        assert hip.hipHostMalloc(C.byref(pinned), C.c_size_t(8 * vv2.size), C.c_uint(0)) == 0
        try:
            C.memmove(pinned, vv2.ctypes.data, 8 * vv2.size)
            assert lib.dav_update_operator_values_dev(e.h, OP_A, pinned) != 0
            assert "vals is not device memory" in lib.dav_last_error().decode()
        finally:
            hip.hipHostFree(pinned)
        # a device allocation one element short: the runtime knows its length, the engine refuses before any launch
        short = C.c_void_p()
        need = 8 * vv2.size
        assert hip.hipMalloc(C.byref(short), C.c_size_t(need - 8)) == 0
        try:
            lo, size = C.c_void_p(), C.c_size_t()
            assert hip.hipMemGetAddressRange(C.byref(lo), C.byref(size), short) == 0 and size.value < need
            assert lib.dav_update_operator_values_dev(e.h, OP_A, short) != 0
            assert f"vals holds fewer than the {need} bytes the matrix needs" in lib.dav_last_error().decode()
        finally:
            hip.hipFree(short)
        # a wrong length through Python: refused before the engine is called
        for device in (False, True):
            with pytest.raises(ValueError, match=f"the set call saw {vv2.size} values"):
                update(e, OP_A, vv2[:-1], device)
        with pytest.raises(TypeError):
            update(e, OP_A, vv2.astype(np.float32), True)
        assert same_state(state(e, x), old)
        # and the operator still takes an update
        update(e, OP_A, vv2, True)
        assert not same_state(state(e, x), old)


# ---- 7. front ends -------------------------------------------------------------------------------------------------------------------
def torch_csr(rp, ci, vv, n):
    return torch.sparse_csr_tensor(torch.tensor(rp), torch.tensor(ci.astype(np.int64)), torch.tensor(vv), size=(n, n)).to(DEV)


def torch_bsr(rp, ci, vv, n):
    return torch.sparse_bsr_tensor(torch.tensor(rp), torch.tensor(ci.astype(np.int64)), torch.tensor(vv), size=(n, n)).to(DEV)


@pytest.mark.parametrize("set_dev,upd_dev", SET_UPDATE)
def test_davidson_engine_update_values_csr(set_dev, upd_dev):
    n, lowest = 1501, 4
    rp, ci, vv = coo_to_csr(n, *sparse_dd(n, 71))
    vv2 = new_values(vv)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_sparse(1, rp, ci, vv2)
        ref = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    with fd.DavidsonEngine(n, lowest) as eng:
        if set_dev:
            eng.set_sparse(1, torch_csr(rp, ci, vv, n), keep_map=True)
        else:
            eng.set_sparse(1, rp, ci, vv, keep_map=True)
        first = eng.solve("DPR", 200, 1e-8, want_vectors=False)
        eng.update_values(1, dev(vv2) if upd_dev else vv2)
        got = eng.solve("DPR", 200, 1e-8, want_vectors=False)
        assert got[2] == ref[2] and np.array_equal(bits(got[0]), bits(ref[0])) and not np.array_equal(first[0], got[0])
        with pytest.raises(ValueError):
            eng.update_values(1, vv2[1:])
        eng.set_sparse(1, rp, ci, vv)                       # keep_map defaults to off: the map goes with the old operator
        with pytest.raises(DavidsonHipError, match="dav_keep_value_map"):
            eng.update_values(1, vv2)


@pytest.mark.parametrize("set_dev,upd_dev", SET_UPDATE)
def test_davidson_engine_update_values_bsr(set_dev, upd_dev):
    """the host door takes the blocks in Fortran order, the device door row-major: update_values turns (nnzb, b, b) row-major data into
    what the operator was set from"""
    b, nb, lowest = 3, 400, 4
    n = nb * b
    rng = np.random.default_rng(72)
    bi, bj, blk = symmetric_blocks(nb, b, rng, "random")
    rp, ci, vv = sorted_bsr_input(nb, bi, bj, blk, True, BSR_ROW_MAJOR)
    vv2 = new_values(vv)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_block_sparse(1, rp, ci, vv2, lower=True)
        ref = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    with fd.DavidsonEngine(n, lowest) as eng:
        if set_dev:
            eng.set_block_sparse(1, torch_bsr(rp, ci, vv, n), lower=True, keep_map=True)
        else:
            eng.set_block_sparse(1, rp, ci, vv, lower=True, keep_map=True)
        data = vv2 if set_dev == upd_dev else vv2.reshape(-1)
        eng.update_values(1, dev(data) if upd_dev else data)
        got = eng.solve("DPR", 200, 1e-8, want_vectors=False)
        assert got[2] == ref[2] and np.array_equal(bits(got[0]), bits(ref[0]))


def test_sparse_refresh_fortran_program_matches_the_oracle(tmp_path):
    from oracle import davidson_oracle as O
    from test_fortran_programs import _run
    from test_sparse_refresh_cpu import build_sparse_refresh_program
    rc, out = _run(build_sparse_refresh_program(tmp_path))
    assert rc == 0, out
    checks = re.findall(r"CHECK (\S+) ([TF])", out)
    assert len(checks) == 3 and all(v == "T" for _, v in checks), out
    n, lowest = 1200, 4
    spectra = {}
    for label, (d0, dstep, eps) in (("EVALS_FIRST", (1.0, 1.0, 0.3)), ("EVALS_SECOND", (2.0, 1.5, 0.2))):
        a = np.diag(d0 + dstep * np.arange(n))
        for off, w in ((1, eps), (2, 0.5 * eps)):
            a += w * (np.eye(n, k=off) + np.eye(n, k=-off))
        lam_o, _, _ = O.generalized_eigensolver_dense(np.asfortranarray(a), lowest, "DPR", 1000, 1e-8, 10 * lowest, None)
        spectra[label] = np.array([float(v) for v in re.search(label + r"(.*)", out).group(1).split()])
        print(label, spectra[label], "oracle", lam_o, "difference", np.abs(spectra[label] - lam_o).max())
        assert np.abs(spectra[label] - lam_o).max() < 1e-8, label
