"""BSR operators built on the GPU from device block arrays (dav_set_operator_bsr_dev): the storage equals what the host entry
dav_set_operator_bsr builds from the same arrays, so the diagonal, the applies and the solves agree bit for bit - over block sizes,
four kinds of matrix, the four storages of test_bsr_gpu.py, three pairs of index widths, blocks sorted and shuffled within their block
rows; three ranks with straddling block rows; generalized problems and replacement; every array-level refusal of the host entry given
as device arrays; the torch front ends; N = 10^6; the Fortran program."""
import ctypes as C
import re
import threading

import numpy as np
import pytest
import torch

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import BSR_COL_MAJOR, BSR_ROW_MAJOR, OP_A, PANEL_V, PANEL_W, DavidsonHipError
from test_bsr_gpu import BS, STORAGES, banded, block_dd, blocks_to_bsr, bsr_input, bsr_of_dense, put_apply_get, symmetric_blocks
from test_sparse_device_gpu import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ("random", "arrowhead", "no_diagonal", "split_diagonal")
WIDTHS = [(torch.int64, torch.int64), (torch.int32, torch.int32), (torch.int64, torch.int32)]


def blocks_of(nb, b, rng, kind):
    """block triples of the four kinds: the two of symmetric_blocks, and "random" with some diagonal blocks removed (the diagonal is
    0 there) or split into two terms (duplicate diagonal blocks, summed in input order)"""
    if kind in ("random", "arrowhead"):
        return symmetric_blocks(nb, b, rng, kind)
    bi, bj, blk = symmetric_blocks(nb, b, rng, "random")
    on = bi == bj
    if kind == "no_diagonal":
        keep = ~(on & (bi % 5 == 2))
        return bi[keep], bj[keep], blk[keep]
    sel = on & (bi % 3 == 0)
    return (np.concatenate([bi, bi[sel]]), np.concatenate([bj, bj[sel]]),
            np.concatenate([np.where(sel[:, None, None], 0.75 * blk, blk), 0.25 * blk[sel]]))


def sorted_bsr_input(nb, bi, bj, blk, lower, layout):
    """bsr_input with the blocks of every block row in block-column order (duplicates in their given order)"""
    if lower:
        sel = bj <= bi
        bi, bj, blk = bi[sel], bj[sel], blk[sel]
    order = np.lexsort((bj, bi))
    rp, ci, vv = blocks_to_bsr(nb, bi[order], bj[order], blk[order])
    if layout == BSR_COL_MAJOR:
        vv = np.ascontiguousarray(vv.transpose(0, 2, 1))
    return rp, ci, vv


def to_dev(rp, ci, vv, base=0, rp_dtype=torch.int64, ci_dtype=torch.int32):
    return (torch.tensor(rp + base, dtype=rp_dtype, device=DEV), torch.tensor(ci.astype(np.int64) + base, dtype=ci_dtype, device=DEV),
            torch.tensor(vv, dtype=torch.float64, device=DEV))


def both_entries(n, rp, ci, vv, base, lower, layout, widths, x, solve=True):
    """(diagonal, 16-column apply, 64-column apply, eigenvalues, iterations) through the host entry and through the device entry"""
    dev = to_dev(rp, ci, vv, base, *widths)
    out = []
    for device in (False, True):
        def put(e):
            if device:
                e.set_operator_bsr_dev(OP_A, *dev, base=base, lower=lower, layout=layout)
            else:
                e.set_operator_bsr(OP_A, rp + base, ci + base, vv, base=base, lower=lower, layout=layout)
        with fd.CEngine(n=n, max_cols=64) as e:
            put(e)
            d = e.get_diagonal(OP_A)
            y16, y64 = put_apply_get(e, x, 16), put_apply_get(e, x, 64)
        lam, it = np.zeros(0), 0
        if solve:
            with fd.DavidsonEngine(n, 3) as eng:
                put(eng.c)
                lam, _, it = eng.solve("DPR", 60, 1e-8, want_vectors=False)
        out.append((d, y16, y64, lam, it))
    return out


def assert_same(out, what):
    (d0, a0, b0, l0, i0), (d1, a1, b1, l1, i1) = out
    assert np.array_equal(bits(d0), bits(d1)), what
    assert np.array_equal(bits(a0), bits(a1)), what
    assert np.array_equal(bits(b0), bits(b1)), what
    assert i0 == i1 and np.array_equal(bits(l0), bits(l1)), (what, i0, i1, l0, l1)


# ---- 1. bitwise equality with the host entry --------------------------------------------------------------------------------------
# Per kind the eight block sizes walk through the four storages (twice, once sorted and once shuffled), the three width pairs and both
# orders: every b, storage, width pair and order meets every kind.
def _cases():
    for ki, kind in enumerate(KINDS):
        for i, b in enumerate(BS):
            j = i + ki
            yield kind, b, j % 4, j % 3, (j // 4 + j) % 2 == 1
    # block row 0 of the arrowhead longer than the LDS sort tile (2048 keys), out of order: tiles sorted, then merged
    yield "arrowhead_long", 4, 0, 0, True
    yield "arrowhead_long", 4, 3, 2, True


@pytest.mark.parametrize("kind,b,storage,width,shuffled", list(_cases()))
def test_device_build_equals_the_host_build(kind, b, storage, width, shuffled):
    lower, base, layout = STORAGES[storage]
    nb = 4096 if kind == "arrowhead_long" else 150 if kind == "arrowhead" else 61       # arrowhead: block row 0 > BSR_CHUNK blocks
    n = nb * b
    rng = np.random.default_rng(1000 * KINDS.index(kind.split("_long")[0]) + 10 * b + storage)
    bi, bj, blk = blocks_of(nb, b, rng, kind.split("_long")[0])
    if shuffled:
        rp, ci, vv = bsr_input(nb, bi, bj, blk, lower, layout, rng)
    else:
        rp, ci, vv = sorted_bsr_input(nb, bi, bj, blk, lower, layout)
    if kind == "arrowhead_long":
        assert np.diff(rp).max() + (nb if lower else 0) > 2048          # more blocks in block row 0 than the LDS sort tile holds
    x = rng.standard_normal((n, 64))
    # without some diagonal blocks the preconditioner meets zeros of the diagonal: the solve is left to the other kinds
    out = both_entries(n, rp, ci, vv, base, lower, layout, WIDTHS[width], x, solve=kind != "no_diagonal")
    assert_same(out, (kind, b, storage, width, shuffled))
    if kind == "no_diagonal":
        assert (out[1][0].reshape(nb, b)[np.arange(nb) % 5 == 2] == 0).all()


@pytest.mark.parametrize("storage", [0, 1, 2, 3])
def test_signed_zeros_and_nan_payloads_are_moved_not_recomputed(storage):
    lower, base, layout = STORAGES[storage]
    b, nb = 4, 61
    n = nb * b
    rng = np.random.default_rng(7 + storage)
    bi, bj, blk = symmetric_blocks(nb, b, rng, "random")
    rp, ci, vv = bsr_input(nb, bi, bj, blk, lower, layout, rng)
    rows = np.repeat(np.arange(nb), np.diff(rp))
    p = int(np.flatnonzero(ci < rows)[5])                      # a strict lower block: mirrored with lower storage
    vv[p, 0, 1] = -0.0
    vv[p, 2, 1] = np.array([0x7FF8000000000ABC], dtype=np.uint64).view(np.float64)[0]
    vv[p, 3, 0] = np.array([0xFFF800000000F00D], dtype=np.uint64).view(np.float64)[0]
    assert bits(vv[p, 2, 1:2])[0] == 0x7FF8000000000ABC
    I, J = int(rows[p]), int(ci[p])
    x = np.zeros((n, 64))
    for c in range(b):                                          # unit vectors over the columns of the block and of its mirror
        x[J * b + c, c] = 1.0
        x[I * b + c, b + c] = 1.0
    out = both_entries(n, rp, ci, vv, base, lower, layout, WIDTHS[storage % 3], x, solve=False)
    assert_same(out, storage)
    y = out[1][1]
    assert np.isnan(y[I * b:(I + 1) * b, :b]).any()             # the marked block took part in the product


# ---- 2. ranks ---------------------------------------------------------------------------------------------------------------------
# N = 1050 on three ranks: slabs of 352 rows, so block rows of b = 3, 5, 6, 7 (and of b = 12 at N = 1056) straddle two ranks
@pytest.mark.parametrize("b,n,kind", [(3, 1050, "random"), (5, 1050, "random"), (6, 1050, "random"), (7, 1050, "random"),
                                      (12, 1056, "random"), (3, 1050, "arrowhead")])
def test_three_ranks_with_their_own_device_copies_equal_one_rank(b, n, kind):
    nranks, nb = 3, n // b
    rng = np.random.default_rng(200 + b)
    bi, bj, blk = symmetric_blocks(nb, b, rng, kind)
    rp, ci, vv = bsr_input(nb, bi, bj, blk, True, BSR_ROW_MAJOR, rng)
    x = rng.standard_normal((n, 64))
    with fd.CEngine(n=n, max_cols=64) as e:
        e.set_operator_bsr(OP_A, rp, ci, vv, lower=True)
        y1 = put_apply_get(e, x, 64)
    engs = [fd.CEngine(n=n, max_cols=64, rank=r, nranks=nranks) for r in range(nranks)]
    copies = [to_dev(rp, ci, vv) for _ in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def work(r):
        try:
            engs[r].set_operator_bsr_dev(OP_A, *copies[r], lower=True)
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


# ---- 3. generalized problems and replacement ----------------------------------------------------------------------------------------
def torch_bsr(rp, ci, vv, n, device=DEV):
    return torch.sparse_bsr_tensor(torch.tensor(rp, dtype=torch.int64), torch.tensor(ci.astype(np.int64)), torch.tensor(vv),
                                   size=(n, n)).to(device)


def csr_of_dense(a):
    n = a.shape[0]
    rows, cols = np.nonzero(a)
    indptr = np.searchsorted(rows, np.arange(n + 1)).astype(np.int64)
    return indptr, cols.astype(np.int32), np.ascontiguousarray(a[rows, cols])


def test_generalized_pair_replacement_and_mixed_inputs():
    n, b, lowest = 1200, 4, 4
    am, bm, om = block_dd(n, b, 61), banded(n, 1.0, 0.0, 0.05), block_dd(n, b, 63)
    a, bb, other = bsr_of_dense(am, b), bsr_of_dense(bm, b), bsr_of_dense(om, b)

    def run(set_a, set_b):
        with fd.DavidsonEngine(n, lowest, gev=True) as eng:
            set_a(eng)
            set_b(eng)
            return eng.solve("DPR", 200, 1e-8, want_vectors=False)

    host_a = lambda eng: eng.set_block_sparse(1, *a)                       # noqa: E731
    dev_a = lambda eng: eng.set_block_sparse(1, torch_bsr(*a, n))          # noqa: E731
    ref = run(host_a, lambda eng: eng.set_block_sparse(2, *bb))
    ref_csr = run(host_a, lambda eng: eng.set_sparse(2, *csr_of_dense(bm)))
    ref_dense = run(host_a, lambda eng: eng.set_dense(2, bm))

    def device_after_host(eng):
        eng.set_block_sparse(1, *other)
        eng.set_block_sparse(1, torch_bsr(*a, n))

    def host_after_device(eng):
        eng.set_block_sparse(1, torch_bsr(*other, n))
        eng.set_block_sparse(1, *a)

    runs = [(run(dev_a, lambda eng: eng.set_block_sparse(2, torch_bsr(*bb, n))), ref, "A and B device"),
            (run(dev_a, lambda eng: eng.set_block_sparse(2, *bb)), ref, "B host BSR"),
            (run(dev_a, lambda eng: eng.set_sparse(2, *csr_of_dense(bm))), ref_csr, "B host CSR"),
            (run(dev_a, lambda eng: eng.set_dense(2, bm)), ref_dense, "B dense"),
            (run(device_after_host, lambda eng: eng.set_block_sparse(2, torch_bsr(*bb, n))), ref, "device after host"),
            (run(host_after_device, lambda eng: eng.set_block_sparse(2, torch_bsr(*bb, n))), ref, "host after device")]
    for got, want, what in runs:
        assert 0 < want[2] < 200
        assert got[2] == want[2] and np.array_equal(bits(got[0]), bits(want[0])), (what, got, want)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def _suffix(msg):
    return re.sub(r"^dav_set_operator_bsr(_dev)?: ", "", msg)


def test_refusals_match_the_host_entry_and_leave_the_engine_usable():
    n, b = 480, 4
    nb = n // b
    a = block_dd(n, b, 51)
    rp, ci, vv = bsr_of_dense(a, b)
    lrp, lci, lvv = bsr_of_dense(a, b, lower=True)
    bad_rp = rp.copy()
    bad_rp[50] = bad_rp[52]
    bad_rp[90] = bad_rp[92]                                  # two places: the first is named
    bad_ci = ci.copy()
    bad_ci[[17, 200, 333]] = [nb, -1, nb + 5]
    neg_ci = ci.copy()
    neg_ci[3] = -1
    cases = [((bad_rp, ci, vv), {}, "block_row_ptr decreases at block row 50"),
             ((rp, bad_ci, vv), {}, f"block column {nb} out of range at block 17"),
             ((rp, neg_ci, vv), {}, "block column -1 out of range at block 3 (block row 0)"),
             ((rp, ci, vv), {"lower": True}, "lies above the diagonal of a DAV_CSR_LOWER matrix"),
             ((rp + 1, ci + 1, vv), {}, "must equal the index base 0"),
             ((rp, ci, vv), {"base": 1}, "block_row_ptr[0] = 0 must equal the index base 1"),
             ((rp, ci, vv), {"base": 2}, "index_base must be 0 or 1"),
             ((rp, ci, vv), {"layout": 2}, "block_layout must be")]
    lib = fd.hip_lib()
    with fd.CEngine(n=n, max_cols=16) as e:
        for (r, c, v), kw, words in cases:
            with pytest.raises(DavidsonHipError) as host:
                if "layout" in kw:             # (the numpy front end checks the layout itself: straight to the C entry)
                    rc = lib.dav_set_operator_bsr(e.h, C.c_int(OP_A), C.c_int(b), r.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  c.ctypes.data_as(C.POINTER(C.c_int32)), v.ctypes.data_as(C.POINTER(C.c_double)),
                                                  C.c_int(0), C.c_int(0), C.c_int(kw["layout"]))
                    assert rc != 0
                    raise DavidsonHipError(lib.dav_last_error().decode())
                e.set_operator_bsr(OP_A, r, c, v, **kw)
            assert words in str(host.value)
            for rpt, cit in WIDTHS:
                dev = (torch.tensor(r, dtype=rpt, device=DEV), torch.tensor(c.astype(np.int64), dtype=cit, device=DEV),
                       torch.tensor(v, device=DEV))
                with pytest.raises(DavidsonHipError) as got:
                    e.set_operator_bsr_dev(OP_A, *dev, **kw)
                assert str(got.value).startswith("dav_set_operator_bsr_dev: ")
                assert _suffix(str(got.value)) == _suffix(str(host.value))
                with pytest.raises(DavidsonHipError, match="operator not set"):
                    e.apply(OP_A, PANEL_V, 0, 1, PANEL_W, 0)
        # arguments the torch front end cannot produce: straight to the C entry
        d_rp, d_ci, d_vv = to_dev(rp, ci, vv)
        p = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
        raw = [((0, p(d_rp), 64, p(d_ci), 32, p(d_vv), 0, 0, 0), "block_size = 0 must lie in 1..16"),
               ((17, p(d_rp), 64, p(d_ci), 32, p(d_vv), 0, 0, 0), "block_size = 17 must lie in 1..16"),
               ((7, p(d_rp), 64, p(d_ci), 32, p(d_vv), 0, 0, 0), "n = 480 is not a multiple of block_size = 7"),
               ((b, p(d_rp), 48, p(d_ci), 32, p(d_vv), 0, 0, 0), "row_ptr_bits must be 32 or 64"),
               ((b, p(d_rp), 64, p(d_ci), 16, p(d_vv), 0, 0, 0), "col_bits must be 32 or 64"),
               ((b, p(d_rp), 64, p(d_ci), 32, p(d_vv), 0, 7, 0), "triangle must be DAV_CSR_FULL or DAV_CSR_LOWER"),
               ((b, None, 64, p(d_ci), 32, p(d_vv), 0, 0, 0), "null block_row_ptr"),
               ((b, p(d_rp), 64, None, 32, p(d_vv), 0, 0, 0), "null block_col_idx or vals"),
               ((b, p(d_rp), 64, p(d_ci), 32, None, 0, 0, 0), "null block_col_idx or vals")]
        for args, msg in raw:
            assert lib.dav_set_operator_bsr_dev(e.h, OP_A, *args) != 0
            assert _suffix(lib.dav_last_error().decode()) == msg
        # host memory holding valid arrays - pageable (numpy, a CPU tensor) and pinned: refused by the pointer check, never read by a kernel
        cpu_vv = torch.tensor(vv)
        hip = C.CDLL("libamdhip64.so")
        pinned = C.c_void_p()
        assert hip.hipHostMalloc(C.byref(pinned), C.c_size_t(8 * (nb + 1)), C.c_uint(0)) == 0
        try:
            C.memmove(pinned, rp.ctypes.data, 8 * (nb + 1))
            for args, name in [((b, C.c_void_p(rp.ctypes.data), 64, p(d_ci), 32, p(d_vv), 0, 0, 0), "block_row_ptr"),
                               ((b, pinned, 64, p(d_ci), 32, p(d_vv), 0, 0, 0), "block_row_ptr"),
                               ((b, p(d_rp), 64, C.c_void_p(ci.ctypes.data), 32, p(d_vv), 0, 0, 0), "block_col_idx"),
                               ((b, p(d_rp), 64, p(d_ci), 32, C.c_void_p(cpu_vv.data_ptr()), 0, 0, 0), "vals")]:
                assert lib.dav_set_operator_bsr_dev(e.h, OP_A, *args) != 0
                assert f"{name} is not device memory" in lib.dav_last_error().decode()
        finally:
            hip.hipHostFree(pinned)
        # an allocation of half the values: the runtime knows its length (asked first, here), the engine refuses before any launch
        short = C.c_void_p()
        need = 8 * b * b * ci.size
        assert hip.hipMalloc(C.byref(short), C.c_size_t(need // 2)) == 0
        try:
            lo, size = C.c_void_p(), C.c_size_t()
            assert hip.hipMemGetAddressRange(C.byref(lo), C.byref(size), short) == 0 and size.value < need
            assert lib.dav_set_operator_bsr_dev(e.h, OP_A, b, p(d_rp), 64, p(d_ci), 32, short, 0, 0, 0) != 0
            assert f"vals holds fewer than the {need} bytes the matrix needs" in lib.dav_last_error().decode()
        finally:
            hip.hipFree(short)
        with pytest.raises(ValueError, match="row_ptr says"):
            e.set_operator_bsr_dev(OP_A, d_rp, d_ci, d_vv[:-1])
        with pytest.raises(DavidsonHipError, match="operator not set"):
            e.apply(OP_A, PANEL_V, 0, 1, PANEL_W, 0)
        # the engine then takes a valid matrix
        e.set_operator_bsr_dev(OP_A, *to_dev(lrp, lci, lvv, 0, torch.int64, torch.int64), lower=True)
        x = np.random.default_rng(1).standard_normal((n, 8))
        y = put_apply_get(e, x, 8)
        assert np.abs(y - a @ x).max() < 1e-12
        e.set_operator_bsr(OP_A, lrp, lci, lvv, lower=True)
        assert np.array_equal(bits(y), bits(put_apply_get(e, x, 8)))


# ---- 5. Python and torch -------------------------------------------------------------------------------------------------------------
def test_torch_front_ends_match_numpy_input():
    n, b, lowest = 2000, 8, 4
    rp, ci, vv = bsr_of_dense(block_dd(n, b, 71), b)
    x = np.random.default_rng(2).standard_normal((n, 16))
    with fd.CEngine(n=n, max_cols=16) as e:
        e.set_operator_bsr(OP_A, rp, ci, vv)
        y = put_apply_get(e, x, 16)
        e.set_operator_bsr(OP_A, torch_bsr(rp, ci, vv, n))
        assert np.array_equal(bits(y), bits(put_apply_get(e, x, 16)))
        e.set_operator_bsr(OP_A, torch_bsr(rp, ci, vv, n, "cpu"))
        assert np.array_equal(bits(y), bits(put_apply_get(e, x, 16)))
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_block_sparse(1, rp, ci, vv)
        ref = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_block_sparse(1, torch_bsr(rp, ci, vv, n))
        got = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    assert 0 < ref[2] < 200 and got[2] == ref[2] and np.array_equal(bits(got[0]), bits(ref[0]))
    second = bsr_of_dense(banded(n, 1.0, 0.0, 0.05), b)
    for sec_h, sec_d in ((None, None), (second, torch_bsr(*second, n))):
        lam_h, _, it_h = fd.generalized_eigensolver_bsr(rp, ci, vv, lowest, "DPR", 200, 1e-8, second=sec_h)
        lam_d, vec_d, it_d = fd.generalized_eigensolver_bsr(torch_bsr(rp, ci, vv, n), None, None, lowest, "DPR", 200, 1e-8, second=sec_d)
        assert it_d == it_h and np.array_equal(bits(lam_d), bits(lam_h)), (it_d, it_h, lam_d, lam_h)
        assert vec_d.shape == (n, lowest)


def test_torch_dtype_and_refusal_errors():
    n, b = 320, 4
    rp, ci, vv = bsr_of_dense(block_dd(n, b, 81), b)
    with fd.DavidsonEngine(n, 2) as eng:
        t32 = torch.sparse_bsr_tensor(torch.tensor(rp), torch.tensor(ci.astype(np.int64)), torch.tensor(vv, dtype=torch.float32),
                                      size=(n, n)).to(DEV)
        with pytest.raises(TypeError):
            eng.set_block_sparse(1, t32)
        with pytest.raises(DavidsonHipError, match="lies above the diagonal"):
            eng.set_block_sparse(1, torch_bsr(rp, ci, vv, n), lower=True)    # a full matrix given as lower: refused, the process lives on
        with pytest.raises(DavidsonHipError, match="operator not set"):
            eng.c.apply(OP_A, PANEL_V, 0, 1, PANEL_W, 0)
        eng.set_block_sparse(1, torch_bsr(rp, ci, vv, n))
        lam, _, it = eng.solve("DPR", 200, 1e-8, want_vectors=False)
        assert 0 < it < 200


# ---- 6. full order ------------------------------------------------------------------------------------------------------------------
def test_a_million_rows_in_8x8_blocks_lower_from_torch_device_tensors():
    """N = 10^6, b = 8, a block band of half-width 4 given as its lower block triangle: the device-built operator solves as the
    host-built one does"""
    n, b, lowest, half = 1_000_000, 8, 16, 4
    nb = n // b
    I = np.arange(nb, dtype=np.int64)
    counts = np.minimum(I, half) + 1
    indptr = np.zeros(nb + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    bi = np.repeat(I, counts)
    bj = np.maximum(I - half, 0)[bi] + (np.arange(indptr[-1], dtype=np.int64) - indptr[bi])
    r = bi[:, None, None] * b + np.arange(b)[None, :, None]
    c = bj[:, None, None] * b + np.arange(b)[None, None, :]
    d = np.abs(r - c)
    vals = np.where(d == 0, 1.0 + r.astype(np.float64), 1e-2 / (1.0 + d))
    del r, c, d, bi
    cols = bj.astype(np.int32)
    res = []
    for device in (False, True):
        with fd.DavidsonEngine(n, lowest) as eng:
            if device:
                eng.c.set_operator_bsr_dev(OP_A, torch.from_numpy(indptr).to(DEV), torch.from_numpy(cols).to(DEV),
                                           torch.from_numpy(vals).to(DEV), lower=True)
            else:
                eng.c.set_operator_bsr(OP_A, indptr, cols, vals, lower=True)
            res.append(eng.solve("DPR", 100, 1e-8, want_vectors=False))
    (l0, _, i0), (l1, _, i1) = res
    assert 0 < i0 < 100 and i0 == i1 and np.array_equal(bits(l0), bits(l1))


# ---- 7. the Fortran program ---------------------------------------------------------------------------------------------------------
def test_bsr_device_fortran_program_matches_the_host_solve(tmp_path):
    from test_bsr_device_cpu import build_bsr_device_program
    from test_fortran_programs import _run
    rc, out = _run(build_bsr_device_program(tmp_path))
    assert rc == 0, out
    checks = re.findall(r"CHECK (\S+) ([TF])", out)
    assert len(checks) == 5 and all(v == "T" for _, v in checks), out
    host = re.search(r"EVALS_HOST(.*)", out).group(1).split()
    dev = re.search(r"EVALS_DEV(.*)", out).group(1).split()
    assert host == dev and len(host) == 4, out
