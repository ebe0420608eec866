"""GPU: warm starts.  Part one drives the ingest kernel through dav_set_guess / dav_set_guess_dev and reads the X panel back: bit for bit
the caller's array for every size, leading dimension, column count and alignment the kernel distinguishes, on one rank and on three,
and every refusal leaves the engine as it was.  Part two solves: with nothing staged the feature is inert (bitwise), an exact guess
converges in the first iteration where a cold solve does not - through the dense, CSR and BSR entries, both methods, the generalized
problem, every policy and the device-side Rayleigh-Ritz - and the re-solve loop, degenerate guesses, three ranks and host callbacks
reach the eigenvalues of numpy.linalg.eigh."""
import ctypes as C
import functools
import os
import re
import threading

import numpy as np
import pytest
import torch

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import DEVICE_APPLY_FN, OP_A, PANEL_S, PANEL_V, PANEL_X, DavidsonHipError

pytestmark = pytest.mark.gpu
TOL = 1e-8


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- part one: the ingest kernel, exact ------------------------------------------------------------------------------------------------
def guess_values(n, ncols, seed):
    """normal numbers with signed zeros, subnormals and huge / tiny magnitudes among them; every column keeps a non-zero"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, ncols))
    special = np.array([0.0, -0.0, 5e-324, -2.2e-308, 1.7e308, -1e-300])
    mask = rng.random((n, ncols)) < 0.2
    x[mask] = rng.choice(special, size=int(mask.sum()))
    x[rng.integers(0, n, ncols), np.arange(ncols)] = rng.standard_normal(ncols) + 3.0
    return x


def strided(x, ldx, lead=0):
    """x(n, ncols) laid out column-major with leading dimension ldx behind `lead` doubles; the gaps hold NaN (never to be read as data)"""
    n, ncols = x.shape
    flat = np.full(lead + ldx * (ncols - 1) + n, np.nan)
    for c in range(ncols):
        flat[lead + c * ldx: lead + c * ldx + n] = x[:, c]
    return flat


LDX = (lambda n: n, lambda n: n + 1, lambda n: n + 3 if (n + 3) % 2 else n + 2, lambda n: 2 * n)


class PadRows:
    """The pad rows [n, ld) of the engine's X and S panels, which no panel door moves.  The engine hands a caller's device operator the
    address and the leading dimension of the panel it is to fill: an operator that only notes them down gives the test both panels, and
    the HIP runtime reads and writes the rows behind row n there."""

    def __init__(self, e, n):
        self.e, self.n, self.seen = e, n, []
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]

        def note(ctx, stream, nn, row0, nloc, k, x_dev, ldx, y_dev, ldy):
            self.seen.append((y_dev, ldy))
            return 0

        self.fn = DEVICE_APPLY_FN(note)
        e.set_operator_device(OP_A, self.fn, 0, np.ones(n))
        self.addr = {}
        for panel in (PANEL_S, PANEL_X):
            e.apply(OP_A, PANEL_V, 0, 1, panel, 0)
            self.addr[panel], self.ld = self.seen[-1]
        self.npad = self.ld - n
        assert self.npad > 0 and self.addr[PANEL_S] != self.addr[PANEL_X]

    def dirty(self, panel, ncols):
        self.e.synchronize()                                  # (the engine's stream does not wait for the runtime's copies, nor they for it)
        junk = np.full((ncols, self.npad), 7.0)
        assert self.hip.hipMemcpy2D(self.addr[panel] + 8 * self.n, 8 * self.ld, junk.ctypes.data, 8 * self.npad, 8 * self.npad, ncols, 1) == 0

    def read(self, panel, ncols):
        self.e.synchronize()
        out = np.full((ncols, self.npad), np.nan)
        assert self.hip.hipMemcpy2D(out.ctypes.data, 8 * self.npad, self.addr[panel] + 8 * self.n, 8 * self.ld, 8 * self.npad, ncols, 2) == 0
        return out


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 257, 1000])
def test_ingest_is_bitwise_for_every_shape_and_alignment(n):
    with fd.CEngine(n=n, max_cols=80) as e:
        pads = PadRows(e, n)
        pads.dirty(PANEL_X, 8)
        assert (pads.read(PANEL_X, 8) == 7.0).all()          # the door works: what it writes behind row n, it reads back

        def staged_clean(stage, ncols, what):
            """stage() with junk behind row n in both panels: afterwards every pad row of the staged columns is +0.0"""
            pads.dirty(PANEL_S, ncols)
            pads.dirty(PANEL_X, ncols)
            stage()
            assert not bits(pads.read(PANEL_X, ncols)).any(), what
            assert not bits(pads.read(PANEL_S, ncols)).any(), what

        for ncols in (1, 5, 16, 17, 64, 65):
            x = guess_values(n, ncols, 100 * n + ncols)
            for ld in LDX:
                ldx = ld(n)
                flat = strided(x, ldx)
                staged_clean(lambda: e.set_guess_raw(flat, ldx, ncols), ncols, ("host", n, ncols, ldx))
                host = e.panel_get(PANEL_X, 0, ncols)
                assert np.array_equal(bits(host), bits(x)), ("host", n, ncols, ldx)
                assert e.guess_columns() == ncols
                e.panel_put(PANEL_X, 0, np.ones((n, ncols)))                   # X rewritten: the guess is dropped
                assert e.guess_columns() == 0
                for lead in (0, 1):                                            # lead = 1: a source that is only 8-byte aligned
                    t = torch.from_numpy(strided(x, ldx, lead)).cuda()
                    staged_clean(lambda: e.set_guess_dev_raw(t.data_ptr() + 8 * lead, ldx, ncols), ncols, ("device", n, ncols, ldx, lead))
                    dev = e.panel_get(PANEL_X, 0, ncols)
                    assert np.array_equal(bits(dev), bits(x)), ("device", n, ncols, ldx, lead)
                    assert np.array_equal(bits(dev), bits(host))
            # and through a product over the padded rows: the Gram of a guess whose squares cannot overflow equals numpy's over the n
            # rows (every term is at most 36 or so; n of them: rounding of n eps times the largest entry)
            k = min(ncols, 16)
            y = np.clip(guess_values(n, ncols, 7 * n + ncols), -6.0, 6.0)
            staged_clean(lambda: e.set_guess(y), ncols, ("gram", n, ncols))
            g = e.gram(PANEL_X, 0, k, PANEL_X, 0, k)
            ref = y[:, :k].T @ y[:, :k]
            assert np.abs(g - ref).max() <= 4 * n * np.finfo(float).eps * max(1.0, np.abs(ref).max()), (n, ncols)
        # a torch tensor, whatever its strides: column-major as it is, or a column-major copy
        x = guess_values(n, 5, n)
        for t in (torch.from_numpy(x).cuda(), torch.from_numpy(np.asfortranarray(x)).cuda().t().contiguous().t(),
                  torch.from_numpy(np.asfortranarray(np.vstack([x, x]))).cuda().t().contiguous().t()[:n]):
            e.set_guess(t)
            assert np.array_equal(bits(e.panel_get(PANEL_X, 0, 5)), bits(x))


def on_ranks(engs, work):
    """work(r) on every rank, each a thread of this process on the one GPU (loopback transport)"""
    nranks = len(engs)
    handles = (C.c_void_p * nranks)(*[getattr(e, "c", e).h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def run(r):
        try:
            out[r] = work(r)
        except Exception as exc:      # noqa: BLE001
            err[r] = exc
        finally:
            fd.hip_lib().dav_local_group_yield(getattr(engs[r], "c", engs[r]).h)

    th = [threading.Thread(target=run, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    return out, err


@pytest.mark.parametrize("n", [17, 257, 1000])
def test_three_ranks_each_hold_their_slab(n):
    ncols = 5
    x = guess_values(n, ncols, n)
    ldx = n + 1
    flat = strided(x, ldx)
    t = torch.from_numpy(strided(x, ldx, 1)).cuda()
    bad = x.copy()
    bad[n - 1, 3] = np.nan                                 # in the last rank's rows only: every rank must refuse
    engs = [fd.CEngine(n=n, max_cols=16, rank=r, nranks=3) for r in range(3)]

    def work(r):
        e = engs[r]
        e.set_guess_raw(flat, ldx, ncols)
        host = e.panel_get(PANEL_X, 0, ncols)
        e.set_guess_dev_raw(t.data_ptr() + 8, ldx, ncols)
        dev = e.panel_get(PANEL_X, 0, ncols)
        try:
            e.set_guess(bad)
            refused = ""
        except DavidsonHipError as exc:
            refused = str(exc)
        return host, dev, refused, e.guess_columns(), e.panel_get(PANEL_X, 0, ncols)

    out, err = on_ranks(engs, work)
    rows = [e.local_rows() for e in engs]
    for e in engs:
        e.close()
    assert all(v is None for v in err), err
    assert sum(nl for _, nl in rows) == n
    for host, dev, refused, staged, after in out:
        assert np.array_equal(bits(host), bits(x)) and np.array_equal(bits(dev), bits(x))
        assert "not finite" in refused and staged == ncols and np.array_equal(bits(after), bits(x))


@pytest.mark.parametrize("device", [False, True])
def test_refusals_name_the_cause_and_leave_the_engine_as_it_was(device):
    n, ncols = 257, 5
    good = guess_values(n, 3, 1)
    x = guess_values(n, ncols, 2)
    keep = []

    def stage(e, a):
        if device:
            keep.append(torch.from_numpy(np.asfortranarray(a)).cuda())
            e.set_guess_dev_raw(keep[-1].data_ptr(), a.shape[0], a.shape[1])
        else:
            e.set_guess(a)

    with fd.CEngine(n=n, max_cols=16) as e:
        e.panel_put(PANEL_X, 0, guess_values(n, 16, 3))
        stage(e, good)
        before = e.panel_get(PANEL_X, 0, 16)
        assert e.guess_columns() == 3

        def refused(a, match):
            with pytest.raises(DavidsonHipError, match=match):
                stage(e, a)
            assert e.guess_columns() == 3
            assert np.array_equal(bits(e.panel_get(PANEL_X, 0, 16)), bits(before))

        for value in (np.nan, np.inf, -np.inf):
            for i, j in ((0, 0), (n - 1, 2), (100, ncols - 1)):
                bad = x.copy()
                bad[i, j] = value
                refused(bad, "not finite")
        payload = x.copy()
        payload[7, 1] = np.array([0x7ff8dead0000beef], dtype=np.uint64).view(np.float64)[0]
        refused(payload, "not finite")
        assert np.array_equal(bits(e.panel_get(PANEL_S, 0, ncols)), bits(payload))       # the kernel moved the NaN's payload as it is
        for j in (0, ncols - 1):
            bad = x.copy()
            bad[:, j] = np.where(np.arange(n) % 2, 0.0, -0.0)                              # signed zeros are zeros
            refused(bad, f"column {j} of x")
        both = x.copy()
        both[:, [1, 3]] = 0.0
        refused(both, "column 1 of x")                                                     # the first such column
        refused(guess_values(n, 17, 4), "exceeds the engine's max_cols")
        for call, match in ((lambda: e.set_guess_raw(x.T.reshape(-1), n - 1, ncols), "ldx = 256 is smaller than n"),
                            (lambda: e.set_guess_raw(x.T.reshape(-1), n, 0), "ncols = 0"),
                            (lambda: e.set_guess_dev_raw(None, n, ncols), "null pointer"),
                            (lambda: e.set_guess_dev_raw(x.ctypes.data, n, ncols), "x_dev is not device memory")):
            with pytest.raises(DavidsonHipError, match=match):
                call()
            assert e.guess_columns() == 3 and np.array_equal(bits(e.panel_get(PANEL_X, 0, 16)), bits(before))
        # an allocation one double short: the runtime knows its length (asked first, here), the engine refuses before any launch
        hip = C.CDLL("libamdhip64.so")
        short, need = C.c_void_p(), 8 * n * ncols
        assert hip.hipMalloc(C.byref(short), C.c_size_t(need - 8)) == 0
        try:
            lo, size = C.c_void_p(), C.c_size_t()
            assert hip.hipMemGetAddressRange(C.byref(lo), C.byref(size), short) == 0 and size.value < need
            with pytest.raises(DavidsonHipError, match=f"x_dev holds fewer than the {need} bytes"):
                e.set_guess_dev_raw(short.value, n, ncols)
        finally:
            hip.hipFree(short)
        assert e.guess_columns() == 3 and np.array_equal(bits(e.panel_get(PANEL_X, 0, 16)), bits(before))
        pinned = torch.ones((ncols, n), dtype=torch.float64).pin_memory()
        with pytest.raises(DavidsonHipError, match="x_dev is not device memory"):
            e.set_guess_dev_raw(pinned.data_ptr(), n, ncols)
        # the staged guess is still usable: it reaches the front of the basis, unit vectors behind it
        e.set_dense_host(OP_A, np.diag(np.arange(n, 0.0, -1.0)))
        idx, g = e.init_basis_guess(6)
        assert g == 3 and list(idx) == [0, 0, 0, n, n - 1, n - 2] and e.guess_columns() == 0
        v = e.panel_get(PANEL_V, 0, 6)
        assert np.array_equal(bits(v[:, :3]), bits(good)) and np.array_equal(v[:, 3:], np.eye(n)[:, [n - 1, n - 2, n - 3]])


# ---- part two: solves ------------------------------------------------------------------------------------------------------------------
N, B4 = 400, 4


@functools.lru_cache(maxsize=None)
def problem(seed=0, gev=False):
    """block-tridiagonal symmetric A (blocks of 4, full inside the blocks) with an ascending diagonal, B SPD and diagonally dominant on
    the same pattern; eigenpairs from numpy (the generalized ones through the Cholesky factor of B)"""
    rng = np.random.default_rng(seed)
    nb = N // B4
    pat = np.kron(np.abs(np.subtract.outer(np.arange(nb), np.arange(nb))) <= 1, np.ones((B4, B4))) > 0
    a = rng.standard_normal((N, N)) * 0.3
    a = np.where(pat, (a + a.T) / 2, 0.0) + np.diag(1.5 * np.arange(1, N + 1))
    if not gev:
        lam, vec = np.linalg.eigh(a)
        return a, None, pat, lam, vec
    b = rng.standard_normal((N, N)) * 0.02
    b = np.where(pat, (b + b.T) / 2, 0.0) + np.eye(N)
    lc = np.linalg.cholesky(b)
    lam, y = np.linalg.eigh(np.linalg.solve(lc, np.linalg.solve(lc, a).T).T)
    return a, b, pat, lam, np.linalg.solve(lc.T, y)


def csr_of(a, pat):
    indptr = np.concatenate([[0], np.cumsum(pat.sum(axis=1))]).astype(np.int64)
    return indptr, np.nonzero(pat)[1].astype(np.int32), a[pat]


def bsr_of(a, pat):
    nb = N // B4
    bp = pat[::B4, ::B4]
    indptr = np.concatenate([[0], np.cumsum(bp.sum(axis=1))]).astype(np.int64)
    bi, bj = np.nonzero(bp)
    data = np.stack([a[B4 * i:B4 * i + B4, B4 * j:B4 * j + B4] for i, j in zip(bi, bj)])
    return indptr, bj.astype(np.int32), data


def set_operator(eng, which, m, pat, entry, keep_map=False):
    if entry == "dense":
        eng.set_dense(which, m)
    elif entry == "csr":
        eng.set_sparse(which, *csr_of(m, pat), keep_map=keep_map)
    else:
        eng.set_block_sparse(which, *bsr_of(m, pat), keep_map=keep_map)


def engine(entry, lowest, gev=False, seed=0, policy=None, device_rr=False, **kw):
    a, b, pat, _, _ = problem(seed, gev)
    eng = fd.DavidsonEngine(N, lowest, gev=gev, **kw)
    set_operator(eng, 1, a, pat, entry)
    if gev:
        set_operator(eng, 2, b, pat, entry)
    if policy:
        eng.set_correction_policy(policy)
    if device_rr:
        eng.set_device_rr(True)
    return eng


def residuals(a, b, lam, vec):
    return np.linalg.norm(a @ vec - (vec if b is None else b @ vec) * lam[None, :], axis=0)


def check(a, b, lam_ref, lam, vec, tol_ev):
    assert np.abs(lam - lam_ref[:lam.size]).max() < tol_ev, np.abs(lam - lam_ref[:lam.size]).max()
    assert (residuals(a, b, lam, vec) < TOL).all(), residuals(a, b, lam, vec)


@pytest.mark.parametrize("entry", ["dense", "csr", "bsr"])
@pytest.mark.parametrize("lowest", [4, 8])
def test_with_nothing_staged_the_feature_is_inert(entry, lowest):
    with engine(entry, lowest) as untouched, engine(entry, lowest) as off:
        off.keep_result_as_guess(False)
        assert off.c.guess_columns() == 0
        first, second = untouched.solve("DPR", 200, TOL), off.solve("DPR", 200, TOL, reuse_vectors=False)
        assert np.array_equal(bits(first[0]), bits(second[0])) and first[2] == second[2] and first[2] > 1
        again = off.solve("DPR", 200, TOL)                   # the result lies in X, the switch is off: cold again
        assert np.array_equal(bits(again[0]), bits(first[0])) and again[2] == first[2]


EXACT = [(entry, lowest, "DPR", False, None, False) for entry in ("dense", "csr", "bsr") for lowest in (4, 8)] + [
    ("dense", 4, "GJD", False, None, False), ("csr", 8, "GJD", False, None, False), ("bsr", 4, "GJD", False, None, False),
    ("dense", 4, "DPR", True, None, False), ("csr", 4, "DPR", True, None, False), ("bsr", 8, "DPR", True, None, False),
    ("csr", 4, "DPR", False, "unconverged", False), ("dense", 8, "GJD", False, "unconverged", False),
    ("csr", 8, "DPR", False, "locking", False), ("bsr", 4, "GJD", False, "locking", False),
    ("dense", 4, "DPR", False, None, True), ("csr", 8, "DPR", False, None, True), ("bsr", 4, "DPR", True, None, True)]


@pytest.mark.parametrize("entry,lowest,method,gev,policy,device_rr", EXACT)
def test_an_exact_guess_converges_in_the_first_iteration(entry, lowest, method, gev, policy, device_rr):
    a, b, pat, lam_ref, vec_ref = problem(0, gev)
    guess = vec_ref[:, :lowest]
    assert residuals(a, b, lam_ref[:lowest], guess).max() < 1e-11 * np.abs(a).max()
    with engine(entry, lowest, gev, policy=policy, device_rr=device_rr) as eng:
        cold = eng.solve(method, 200, TOL)
        assert cold[2] > 1                                   # without the guess the solver has work to do
        check(a, b, lam_ref, cold[0], cold[1], 1e-8)
        lam, vec, iters = eng.solve(method, 200, TOL, initial_vectors=guess)
        assert iters == 1, (iters, cold[2])
        check(a, b, lam_ref, lam, vec, 1e-10)
        assert eng.c.guess_columns() == 0                    # one-shot: consumed


def test_the_one_call_front_ends_take_initial_vectors():
    a, _, pat, lam_ref, vec_ref = problem(0)
    guess = vec_ref[:, :4]
    for call in (lambda **kw: fd.generalized_eigensolver(a, 4, "DPR", 200, TOL, **kw),
                 lambda **kw: fd.generalized_eigensolver_sparse(*csr_of(a, pat), 4, "DPR", 200, TOL, **kw),
                 lambda **kw: fd.generalized_eigensolver_bsr(*bsr_of(a, pat), 4, "DPR", 200, TOL, **kw)):
        cold, warm = call(), call(initial_vectors=guess)
        assert cold[2] > 1 and warm[2] == 1
        check(a, None, lam_ref, warm[0], warm[1], 1e-10)
    ag, bg, _, lam_g, vec_g = problem(0, True)
    cold = fd.generalized_eigensolver(ag, 4, "DPR", 200, TOL, None, bg)
    warm = fd.generalized_eigensolver(ag, 4, "DPR", 200, TOL, None, bg, initial_vectors=torch.from_numpy(vec_g[:, :4].copy()).cuda())
    assert cold[2] > 1 and warm[2] == 1
    check(ag, bg, lam_g, warm[0], warm[1], 1e-10)


def perturbed(a, pat, seed=9):
    rng = np.random.default_rng(seed)
    e = rng.uniform(-1.0, 1.0, a.shape)
    return a + 1e-3 * np.where(pat, (e + e.T) / 2, 0.0)


@pytest.mark.parametrize("lowest,device_values", [(4, False), (8, True)])
def test_resolve_loop_on_a_kept_pattern_reuses_the_vectors(lowest, device_values, capsys):
    a, _, pat, _, _ = problem(0)
    a2 = perturbed(a, pat)
    lam2 = np.linalg.eigvalsh(a2)
    with fd.DavidsonEngine(N, lowest) as eng, fd.DavidsonEngine(N, lowest) as fresh:
        set_operator(eng, 1, a, pat, "csr", keep_map=True)
        first = eng.solve("DPR", 200, TOL)
        vals = csr_of(a2, pat)[2]
        eng.update_values(1, torch.from_numpy(vals).cuda() if device_values else vals)
        lam, vec, warm_iters = eng.solve("DPR", 200, TOL, reuse_vectors=True)
        set_operator(fresh, 1, a2, pat, "csr")
        cold_iters = fresh.solve("DPR", 200, TOL)[2]
        with capsys.disabled():
            print(f"\nre-solve loop, lowest = {lowest}: first solve {first[2]} iterations, after the update warm {warm_iters}, cold {cold_iters}")
        check(a2, None, lam2, lam, vec, 1e-8)
        assert warm_iters <= cold_iters
        assert eng.c.guess_columns() == lowest               # the switch is sticky: this result is the next solve's guess
        assert eng.solve("DPR", 200, TOL)[2] == 1


def degenerate_guesses(lowest):
    _, _, _, _, vec = problem(0)
    a = problem(0)[0]
    order = np.argsort(np.diag(a), kind="stable")
    rng = np.random.default_rng(3)
    return {"two identical columns": np.column_stack([vec[:, 0], vec[:, 0], vec[:, 1]]),
            "the unit vectors of the cold start": np.eye(N)[:, order[:2 * lowest]],
            "one column": vec[:, :1].copy(),
            "a full start basis": vec[:, :2 * lowest] + 1e-3 * rng.standard_normal((N, 2 * lowest)),
            "wider than the start basis": vec[:, :2 * lowest + 3] + 1e-3 * rng.standard_normal((N, 2 * lowest + 3))}


@pytest.mark.parametrize("name", ["two identical columns", "the unit vectors of the cold start", "one column", "a full start basis",
                                  "wider than the start basis"])
@pytest.mark.parametrize("entry,method", [("csr", "DPR"), ("dense", "GJD")])
def test_degenerate_guesses_still_solve(name, entry, method):
    lowest = 4
    a, _, _, lam_ref, _ = problem(0)
    guess = degenerate_guesses(lowest)[name]
    with engine(entry, lowest) as eng:
        lam, vec, iters = eng.solve(method, 300, TOL, initial_vectors=guess)
        check(a, None, lam_ref, lam, vec, 1e-8)
        assert eng.c.guess_columns() == 0


def test_a_one_shot_guess_is_consumed():
    a, _, _, _, vec_ref = problem(0)
    with engine("csr", 4) as eng, engine("csr", 4) as cold_eng:
        cold = cold_eng.solve("DPR", 200, TOL)
        assert eng.solve("DPR", 200, TOL, initial_vectors=vec_ref[:, :4])[2] == 1
        second = eng.solve("DPR", 200, TOL)
        assert np.array_equal(bits(second[0]), bits(cold[0])) and second[2] == cold[2]


@pytest.mark.parametrize("case", ["exact", "resolve"])
def test_three_ranks_agree_with_one(case):
    lowest = 4
    a, _, pat, lam_ref, vec_ref = problem(0)
    a2 = perturbed(a, pat)

    def run(eng):
        if case == "exact":
            set_operator(eng, 1, a, pat, "csr")
            return eng.solve("DPR", 200, TOL, initial_vectors=vec_ref[:, :lowest])
        set_operator(eng, 1, a, pat, "csr", keep_map=True)
        eng.solve("DPR", 200, TOL)
        eng.update_values(1, csr_of(a2, pat)[2])
        return eng.solve("DPR", 200, TOL, reuse_vectors=True)

    with fd.DavidsonEngine(N, lowest) as one:
        ref = run(one)
    engs = [fd.DavidsonEngine(N, lowest, rank=r, nranks=3) for r in range(3)]
    out, err = on_ranks(engs, lambda r: run(engs[r]))
    for e in engs:
        e.close()
    assert all(v is None for v in err), err
    if case == "exact":
        assert ref[2] == 1
    for lam, vec, iters in out:
        assert iters == ref[2] and np.abs(lam - ref[0]).max() < 1e-12
        check(a if case == "exact" else a2, None, lam_ref if case == "exact" else np.linalg.eigvalsh(a2), lam, vec, 1e-8)


def test_host_callback_operators_start_from_the_guess():
    lowest = 4
    a, b, _, lam_ref, vec_ref = problem(0, True)
    args = (lambda x: a @ x, N, lowest, "DPR", 200, TOL, None, lambda x: b @ x)
    cold = fd.solver.generalized_eigensolver_free(*args)
    lam, vec, iters = fd.solver.generalized_eigensolver_free(*args, initial_vectors=vec_ref[:, :lowest])
    assert cold[2] > 1 and iters == 1
    check(a, b, lam_ref, lam, vec, 1e-10)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/flang"), reason="flang not available")
def test_fortran_program_warm_starts(tmp_path):
    """tests/fortran/prog_guess.f90: initial_vectors= next to positional calls with the reference's list, the three engine routines, a
    refusal returned through stat and a cold solve afterwards"""
    from test_fortran_programs import _run
    from test_guess_cpu import build_guess_program
    rc, out = _run(build_guess_program(tmp_path))
    assert rc == 0, out
    checks = re.findall(r"CHECK (\S+) ([TF])", out)
    assert len(checks) == 7 and all(v == "T" for _, v in checks), out
    cold, warm, eng, again, positional, eng_cold = [int(v) for v in re.search(r"ITERS" + r"\s+(\d+)" * 6, out).groups()]
    assert cold > 1 and positional == cold and warm == 1 and eng == 1 and again == eng_cold > 1
