"""CSR operators built on the GPU from device arrays (dav_set_operator_csr_dev): the storage equals what the host entry
dav_set_operator_csr builds from the same matrix, so the diagonal, the applies and the solves agree bit for bit - over the six matrix
classes of test_sparse_gpu.py, full and lower storage, both index bases and index widths, sorted and row-shuffled input; three ranks;
generalized problems and replacement; every refusal of the host entry given as device arrays; the torch front ends; N = 10^6."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest
import torch

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import OP_A, PANEL_V, PANEL_W, DavidsonHipError
from test_sparse_gpu import coo_to_csr, csr_input, sparse_dd, symmetric_coo

pytestmark = pytest.mark.gpu

CLASSES = ("banded", "random", "empty_rows", "missing_diagonal", "duplicates", "arrowhead")
DEV = "cuda:0"


def sorted_csr(n, rows, cols, vals, lower):
    """the CSR arrays with every row in column order (duplicates in their given order)"""
    if lower:
        sel = cols <= rows
        rows, cols, vals = rows[sel], cols[sel], vals[sel]
    order = np.lexsort((cols, rows))
    return coo_to_csr(n, rows[order], cols[order], vals[order])


def shuffled_rows(rp, ci, vv, rng):
    """the same matrix with the entries of every row in a random order"""
    n = rp.size - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    perm = rng.permutation(rows.size)
    return coo_to_csr(n, rows[perm], ci[perm].astype(np.int64), vv[perm])


def to_dev(rp, ci, vv, base, rp_dtype, ci_dtype):
    return (torch.tensor(rp + base, dtype=rp_dtype, device=DEV), torch.tensor(ci.astype(np.int64) + base, dtype=ci_dtype, device=DEV),
            torch.tensor(vv, dtype=torch.float64, device=DEV))


def put_apply_get(e, x, k):
    e.panel_put(PANEL_V, 0, x[:, :k])
    e.apply(OP_A, PANEL_V, 0, k, PANEL_W, 0)
    return e.panel_get(PANEL_W, 0, k)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


WIDTHS = {"64/64": (torch.int64, torch.int64), "32/32": (torch.int32, torch.int32), "64/32": (torch.int64, torch.int32)}


# ---- 1. bitwise equality with the host entry --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CLASSES)
@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("base,widths", [(0, "64/64"), (1, "32/32"), (0, "64/32"), (1, "64/64")])
@pytest.mark.parametrize("shuffled", [False, True])
def test_device_build_equals_the_host_build(kind, lower, base, widths, shuffled):
    n = 20011 if kind == "arrowhead" else 1003          # the shuffled arrowhead row holds n >> 1024 entries
    rng = np.random.default_rng(CLASSES.index(kind) * 10 + lower)
    rows, cols, vals = symmetric_coo(n, kind, rng)
    rp, ci, vv = sorted_csr(n, rows, cols, vals, lower)
    if shuffled:
        rp, ci, vv = shuffled_rows(rp, ci, vv, rng)
    dev = to_dev(rp, ci, vv, base, *WIDTHS[widths])
    x = rng.standard_normal((n, 64))
    out = []
    for device in (False, True):
        def put(e):
            if device:
                e.set_operator_csr_dev(OP_A, *dev, base=base, lower=lower)
            else:
                e.set_operator_csr(OP_A, rp + base, ci + base, vv, base=base, lower=lower)
        with fd.CEngine(n=n, max_cols=64) as e:
            put(e)
            d = e.get_diagonal(OP_A)
            y16, y64 = put_apply_get(e, x, 16), put_apply_get(e, x, 64)
        with fd.DavidsonEngine(n, 3) as eng:
            put(eng.c)
            lam, _, it = eng.solve("DPR", 60, 1e-8, want_vectors=False)
        out.append((d, y16, y64, lam, it))
    (d0, a0, b0, l0, i0), (d1, a1, b1, l1, i1) = out
    assert np.array_equal(bits(d0), bits(d1))
    assert np.array_equal(bits(a0), bits(a1))
    assert np.array_equal(bits(b0), bits(b1))
    assert i0 == i1 and np.array_equal(bits(l0), bits(l1)), (i0, i1, l0, l1)


# ---- 2. ranks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "arrowhead"])
def test_three_ranks_with_their_own_device_copies_equal_one_rank(kind):
    n, nranks = 2999, 3
    rng = np.random.default_rng(17)
    rows, cols, vals = symmetric_coo(n, kind, rng)
    rp, ci, vv = csr_input(n, rows, cols, vals, True, rng)
    x = rng.standard_normal((n, 64))
    with fd.CEngine(n=n, max_cols=64) as e:
        e.set_operator_csr_dev(OP_A, *to_dev(rp, ci, vv, 0, torch.int64, torch.int32), lower=True)
        y1 = put_apply_get(e, x, 64)
    engs = [fd.CEngine(n=n, max_cols=64, rank=r, nranks=nranks) for r in range(nranks)]
    copies = [to_dev(rp, ci, vv, 0, torch.int64, torch.int32) for _ in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def work(r):
        try:
            engs[r].set_operator_csr_dev(OP_A, *copies[r], lower=True)
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
def torch_csr(rp, ci, vv, n, device=DEV):
    return torch.sparse_csr_tensor(torch.tensor(rp, dtype=torch.int64), torch.tensor(ci.astype(np.int64)), torch.tensor(vv),
                                   size=(n, n)).to(device)


def test_generalized_pair_replacement_and_mixed_inputs():
    n, lowest = 1501, 4
    a = coo_to_csr(n, *sparse_dd(n, 61))
    b = coo_to_csr(n, *sparse_dd(n, 62, diag=2.0))
    other = coo_to_csr(n, *sparse_dd(n, 63))
    with fd.DavidsonEngine(n, lowest, gev=True) as eng:
        eng.set_sparse(1, *a)
        eng.set_sparse(2, *b)
        ref = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    with fd.DavidsonEngine(n, lowest, gev=True) as eng:
        eng.set_sparse(1, torch_csr(*other, n))           # replaced by the next call
        eng.set_sparse(1, torch_csr(*a, n))
        eng.set_sparse(2, torch_csr(*b, n))
        dev = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    with fd.DavidsonEngine(n, lowest, gev=True) as eng:
        eng.set_sparse(1, torch_csr(*a, n))
        eng.set_sparse(2, *b)                              # device A, host B
        mixed = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    for got in (dev, mixed):
        assert got[2] == ref[2] and np.array_equal(bits(got[0]), bits(ref[0])), (got, ref)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def _suffix(msg):
    return re.sub(r"^dav_set_operator_csr(_dev)?: ", "", msg)


def test_refusals_match_the_host_entry_and_leave_the_engine_usable():
    n = 500
    rp, ci, vv = coo_to_csr(n, *sparse_dd(n, 51))
    lower_rp, lower_ci, lower_vv = csr_input(n, *sparse_dd(n, 51), True, np.random.default_rng(0))
    bad_rp = rp.copy()
    bad_rp[100] = bad_rp[102]
    bad_rp[300] = bad_rp[302]
    many_ci = ci.copy()
    many_ci[[17, 900, 2000]] = [n, -1, n + 5]          # several columns out of range: the first is named
    neg_ci = ci.copy()
    neg_ci[3] = -1
    cases = [((bad_rp, ci, vv), {}),
             ((rp, many_ci, vv), {}),
             ((rp, neg_ci, vv), {}),
             ((rp, ci, vv), {"lower": True}),
             ((rp + 1, ci + 1, vv), {}),
             ((rp, ci, vv), {"base": 2})]
    with fd.CEngine(n=n, max_cols=16) as e:
        for (r, c, v), kw in cases:
            with pytest.raises(DavidsonHipError) as host:
                e.set_operator_csr(OP_A, r, c, v, **kw)
            for rpt, cit in WIDTHS.values():
                dev = (torch.tensor(r, dtype=rpt, device=DEV), torch.tensor(c.astype(np.int64), dtype=cit, device=DEV),
                       torch.tensor(v, device=DEV))
                with pytest.raises(DavidsonHipError) as got:
                    e.set_operator_csr_dev(OP_A, *dev, **kw)
                assert _suffix(str(got.value)) == _suffix(str(host.value))
                with pytest.raises(DavidsonHipError, match="operator not set"):
                    e.apply(OP_A, PANEL_V, 0, 1, PANEL_W, 0)
        # arguments the torch front end cannot produce: straight to the C entry
        lib = fd.hip_lib()
        d_rp, d_ci, d_vv = (torch.tensor(rp, device=DEV), torch.tensor(ci, device=DEV), torch.tensor(vv, device=DEV))
        p = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
        raw = [((p(d_rp), 48, p(d_ci), 32, p(d_vv), 0, 0), "row_ptr_bits must be 32 or 64"),
               ((p(d_rp), 64, p(d_ci), 16, p(d_vv), 0, 0), "col_bits must be 32 or 64"),
               ((p(d_rp), 64, p(d_ci), 32, p(d_vv), 0, 7), "triangle must be DAV_CSR_FULL or DAV_CSR_LOWER"),
               ((None, 64, p(d_ci), 32, p(d_vv), 0, 0), "null row_ptr"),
               ((p(d_rp), 64, None, 32, p(d_vv), 0, 0), "null col_idx or vals"),
               ((p(d_rp), 64, p(d_ci), 32, None, 0, 0), "null col_idx or vals")]
        for args, msg in raw:
            assert lib.dav_set_operator_csr_dev(e.h, OP_A, *args) != 0
            assert _suffix(lib.dav_last_error().decode()) == msg
        # pinned host memory holding a valid row_ptr: refused by the pointer check, never read by a kernel
        hip = C.CDLL("libamdhip64.so")
        pinned = C.c_void_p()
        assert hip.hipHostMalloc(C.byref(pinned), C.c_size_t(8 * (n + 1)), C.c_uint(0)) == 0
        try:
            C.memmove(pinned, rp.ctypes.data, 8 * (n + 1))
            assert lib.dav_set_operator_csr_dev(e.h, OP_A, pinned, 64, p(d_ci), 32, p(d_vv), 0, 0) != 0
            assert "row_ptr is not device memory" in lib.dav_last_error().decode()
        finally:
            hip.hipHostFree(pinned)
        with pytest.raises(DavidsonHipError, match="operator not set"):
            e.apply(OP_A, PANEL_V, 0, 1, PANEL_W, 0)
        # the engine then takes a valid matrix
        e.set_operator_csr_dev(OP_A, *to_dev(lower_rp, lower_ci, lower_vv, 0, torch.int64, torch.int64), lower=True)
        x = np.random.default_rng(1).standard_normal((n, 8))
        y = put_apply_get(e, x, 8)
        e.set_operator_csr(OP_A, lower_rp, lower_ci, lower_vv, lower=True)
        assert np.array_equal(bits(y), bits(put_apply_get(e, x, 8)))


# ---- 5. Python and torch -------------------------------------------------------------------------------------------------------------
def test_torch_front_ends_match_numpy_input():
    n, lowest = 2003, 4
    rp, ci, vv = coo_to_csr(n, *sparse_dd(n, 71))
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_sparse(1, rp, ci, vv)
        ref = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    with fd.DavidsonEngine(n, lowest) as eng:
        eng.set_sparse(1, torch_csr(rp, ci, vv, n))
        got = eng.solve("DPR", 200, 1e-8, want_vectors=False)
    assert got[2] == ref[2] and np.array_equal(bits(got[0]), bits(ref[0]))
    lam_h, _, it_h = fd.generalized_eigensolver_sparse(rp, ci, vv, lowest, "DPR", 200, 1e-8)
    lam_d, vec_d, it_d = fd.generalized_eigensolver_sparse(torch_csr(rp, ci, vv, n), None, None, lowest, "DPR", 200, 1e-8)
    assert it_d == it_h and np.abs(lam_d - lam_h).max() < 1e-12
    b = coo_to_csr(n, *sparse_dd(n, 72, diag=2.0))
    lam_h, _, it_h = fd.generalized_eigensolver_sparse(rp, ci, vv, lowest, "DPR", 200, 1e-8, second=b)
    lam_d, _, it_d = fd.generalized_eigensolver_sparse(torch_csr(rp, ci, vv, n), None, None, lowest, "DPR", 200, 1e-8,
                                                       second=torch_csr(*b, n))
    assert it_d == it_h and np.abs(lam_d - lam_h).max() < 1e-12


def test_torch_dtype_and_refusal_errors():
    n = 300
    rp, ci, vv = coo_to_csr(n, *sparse_dd(n, 81))
    with fd.DavidsonEngine(n, 2) as eng:
        t32 = torch.sparse_csr_tensor(torch.tensor(rp), torch.tensor(ci.astype(np.int64)), torch.tensor(vv, dtype=torch.float32),
                                      size=(n, n)).to(DEV)
        with pytest.raises(TypeError):
            eng.set_sparse(1, t32)
        with pytest.raises(DavidsonHipError, match="lies above the diagonal"):
            eng.set_sparse(1, torch_csr(rp, ci, vv, n), lower=True)      # a full matrix given as lower: refused, the process lives on
        eng.set_sparse(1, torch_csr(rp, ci, vv, n))
        lam, _, it = eng.solve("DPR", 200, 1e-8, want_vectors=False)
        assert 0 < it < 200


# ---- 7. full order ------------------------------------------------------------------------------------------------------------------
def test_a_million_rows_lower_from_torch_device_tensors():
    """N = 10^6, banded 65 per row given as its lower triangle: the device-built operator solves as the host-built one does"""
    n, lowest, half = 1_000_000, 8, 32
    counts = np.minimum(np.arange(n), half) + 1
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    rows = np.repeat(np.arange(n, dtype=np.int64), counts)
    first = np.maximum(np.arange(n, dtype=np.int64) - half, 0)
    cols = (first[rows] + (np.arange(indptr[-1], dtype=np.int64) - indptr[rows])).astype(np.int32)
    d = rows - cols
    vals = np.where(d == 0, 1.0 + rows.astype(np.float64), 1e-2 / (1.0 + d))
    del d, rows, first
    res = []
    for device in (False, True):
        with fd.DavidsonEngine(n, lowest) as eng:
            if device:
                eng.c.set_operator_csr_dev(OP_A, torch.from_numpy(indptr).to(DEV), torch.from_numpy(cols).to(DEV),
                                           torch.from_numpy(vals).to(DEV), lower=True)
            else:
                eng.c.set_operator_csr(OP_A, indptr, cols, vals, lower=True)
            res.append(eng.solve("DPR", 100, 1e-8, want_vectors=False))
    (l0, _, i0), (l1, _, i1) = res
    assert 0 < i0 < 100 and i0 == i1 and np.array_equal(bits(l0), bits(l1))


# ---- 6. the Fortran program ---------------------------------------------------------------------------------------------------------
def test_sparse_device_fortran_program_matches_the_host_solve(tmp_path):
    from test_fortran_programs import _run
    from test_sparse_device_cpu import build_sparse_device_program
    rc, out = _run(build_sparse_device_program(tmp_path))
    assert rc == 0, out
    checks = re.findall(r"CHECK (\S+) ([TF])", out)
    assert len(checks) == 4 and all(v == "T" for _, v in checks), out
    host = re.search(r"EVALS_HOST(.*)", out).group(1).split()
    dev = re.search(r"EVALS_DEV(.*)", out).group(1).split()
    assert host == dev and len(host) == 4, out
