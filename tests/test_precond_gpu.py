"""GPU: the preconditioner slot (DAV_OP_M) - an operator the caller hands over as an approximation of (A - sigma B)^-1, which the DPR
correction (T = M R) and the GJD correction (the preconditioner of its MINRES) apply in place of the diagonal.
  T1  the DPR phase with M set, inside write fences, on integer data (tests/exact_inputs.py): V[:, m:m+ncorr] is bit for bit what
      dav_apply(DAV_OP_M, DAV_PANEL_R -> DAV_PANEL_S) gives on the R of a DAV_METHOD_NONE phase - and, the data being integers, bit for
      bit the int64 product M R; the residual norms are those of the phase without M; nothing outside the block is written; the _g
      entry's C and G are [V T]^T T bit for bit (the bound of the _g test of tests/test_exact_phases_gpu.py); three ranks give the bits
      of one rank.  M as CSR, BSR (b = 3, 16), DIA, identity and the stencil of lib/test/libuser_operator.so as a device callback.  A BSR
      operator needs n to be a multiple of b: those cases run at the next multiple of b above n.
  T2  BDPR, CHEB and LCHEB do not read the slot.
  T3  GJD: a diagonal M restates the Jacobi run; a dense inverse needs fewer inner steps and solves the correction equations to the
      bound tests/test_solver_gpu.py puts on the Jacobi solve; M = -I is refused with a message naming M, the basis untouched.
  T4  solves: with M at most half the iterations of plain DPR (tests/test_precond_cpu.py holds the numpy restatement to the same
      condition), eigenvalues against numpy.linalg.eigh; the generalized pencil; the policies; three ranks; the stencil as a callback
      against the same matrix as CSR.
  T5  new values on the kept pattern of M give the T of a fresh set call.
  T6  the C entries that refuse the slot name DAV_OP_M and leave the engine usable; slot 3 is still a bad operator id."""
import ctypes as C
import os
import threading
import zlib

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import (METHOD_BDPR, METHOD_CHEB, METHOD_DPR, METHOD_GJD, METHOD_LCHEB, METHOD_NONE, OP_A, OP_B, OP_M, PANEL_BV,
                                           PANEL_R, PANEL_S, PANEL_V, PANEL_W, PANEL_X, DavidsonHipError)
import bdpr_inputs as BI
import precond_inputs as P
from exact_inputs import (SENTINEL, GjdInputs, cols_alloc, dpr_diagonals, fenced, int_product, mismatch, ritz_inputs, ritz_reference,
                          run_ranks, same_bits)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STENCIL = (2.0, 0.0, 2.0)            # d0, dstep, eps of the user operator: the integer entries 2 | 2 | 1


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


@pytest.fixture(scope="module")
def user():
    fd.hip_lib()            # first: one HIP runtime per process (as tests/test_device_operator_gpu.py)
    lib = C.CDLL(os.path.join(ROOT, "fortran_davidson_amd", "lib", "test", "libuser_operator.so"))
    lib.user_op_create.restype = C.c_void_p
    lib.user_op_create.argtypes = [C.c_double, C.c_double, C.c_double]
    lib.user_op_destroy.argtypes = [C.c_void_p]
    return lib


# ---- T1. the DPR phase -----------------------------------------------------------------------------------------------------------------
FORMS = ["csr", "bsr3", "bsr16", "dia", "identity", "stencil"]
T1_NS = [1, 17, 300, 4097]
T1_SHAPES = [(5, 5, 2), (17, 17, 3), (40, 33, 4)]          # m, ncorr, lowest


def rows_of(form, n):
    b = {"bsr3": 3, "bsr16": 16}.get(form, 1)
    return -(-n // b) * b


def m_matrix(form, n):
    """the dense integer M of a form, order n"""
    if form == "identity":
        return np.eye(n)
    if form == "stencil":
        return P.stencil_matrix(n, *STENCIL)
    return P.int_banded(n, _seed("M", form, n))


def set_m(e, form, n, user=None, keep=None):
    a = m_matrix(form, n)
    if form == "csr":
        e.set_operator_csr(OP_M, *P.csr_of(a))
    elif form == "dia":
        e.set_operator_csr(OP_M, *P.csr_of(a), diagonals=True)
    elif form in ("bsr3", "bsr16"):
        e.set_operator_bsr(OP_M, *P.bsr_of(a, int(form[3:])))
    elif form == "identity":
        e.set_operator_identity(OP_M)
    else:
        ctx = user.user_op_create(*STENCIL)
        keep.append(ctx)
        e.set_operator_device(OP_M, user.user_op_apply, ctx, None)
    return a


def dpr_phase(e, n, shape, gev, kind, entry, form, user=None, keep=None, m_is_set=False):
    """The three steps of T1 in one engine, each inside fresh fences: (0) the DPR phase before M is set, for its norms; then, with M
    set, (1) DAV_METHOD_NONE, (2) dav_apply(M, R -> S), (3) the DPR phase.  Returns (messages, T).  m_is_set: the engine has its M
    already (a second case in one engine): step 0 is skipped."""
    m, ncorr, lowest = shape
    cols = e.cols
    rng = np.random.default_rng(_seed("precond ritz", n, shape, gev, kind))
    v, w, z, y, theta = ritz_inputs(kind, n, m, ncorr, gev, rng, dyadic=True)
    xi, ri, ss = ritz_reference(v, w, z, y, theta)
    da, db, _ = dpr_diagonals(n, gev, theta, rng, None)
    src = {PANEL_V: fenced(n, cols, SENTINEL, 0, v), PANEL_W: fenced(n, cols, np.nan, 0, w), PANEL_X: fenced(n, cols, SENTINEL),
           PANEL_R: fenced(n, cols, SENTINEL), PANEL_S: fenced(n, cols, SENTINEL)}
    if gev:
        src[PANEL_BV] = fenced(n, cols, np.nan, 0, z)

    def put():
        for p, a in src.items():
            e.panel_put(p, 0, a)

    def run(method):
        if entry == "g" and method == METHOD_DPR:
            return e.ritz_residual_correction_g(m, ncorr, lowest, y, theta)
        return (e.ritz_residual_correction_n(m, ncorr, lowest, y, theta, method),)

    msgs = []
    norms0 = None
    if not m_is_set:
        e.set_operator_host(OP_A, da)
        if gev:
            e.set_operator_host(OP_B, db)
        put()
        norms0 = run(METHOD_DPR)[0]
        if not same_bits(e.panel_get(PANEL_R, 0, cols), src[PANEL_R]):
            msgs.append("without M the DPR phase wrote the R panel")
        mm = set_m(e, form, n, user, keep)
    else:
        mm = m_matrix(form, n)
    # 1. the residues alone
    put()
    norms_none = run(METHOD_NONE)[0]
    r = e.panel_get(PANEL_R, 0, cols)
    if not same_bits(r[:, :ncorr], ri.astype(np.float64)):
        msgs.append("R of DAV_METHOD_NONE: " + mismatch(r[:, :ncorr], ri.astype(np.float64)))
    # 2. M R through dav_apply
    e.apply(OP_M, PANEL_R, 0, ncorr, PANEL_S, 0)
    s = e.panel_get(PANEL_S, 0, cols)
    t_exact = int_product(mm, ri).astype(np.float64)
    assert (np.abs(t_exact) < 2.0 ** 53).all()
    if not same_bits(s[:, :ncorr], t_exact):
        msgs.append("dav_apply(M, R) against the integer product: " + mismatch(s[:, :ncorr], t_exact))
    if not same_bits(s[:, ncorr:], src[PANEL_S][:, ncorr:]):
        msgs.append("dav_apply(M, R) wrote beyond its columns")
    # 3. the DPR phase
    put()
    out = run(METHOD_DPR)
    got = {p: e.panel_get(p, 0, cols) for p in src}
    exp = {p: a.copy() for p, a in src.items()}
    exp[PANEL_V][:, m:m + ncorr] = s[:, :ncorr]
    exp[PANEL_R][:, :ncorr] = ri
    exp[PANEL_X][:, :lowest] = xi[:, :lowest]
    for p in src:
        if not same_bits(got[p], exp[p]):
            msgs.append(f"panel {p} after the DPR phase: " + mismatch(got[p], exp[p]))
    for what, other in (("the phase without M", norms0), ("DAV_METHOD_NONE", norms_none)):
        if other is not None and not same_bits(out[0], other):
            msgs.append(f"residual norms against those of {what}: {out[0]} vs {other}")
    if entry == "g":
        t = t_exact
        assert (np.sum(t * t, axis=0) < 2.0 ** 53).all()                           # then every order of summation is exact
        for what, a, b in (("C = V^T T", out[1], np.asfortranarray(v.T @ t)), ("G = T^T T", out[2], np.asfortranarray(t.T @ t))):
            if not same_bits(a, b):
                msgs.append(f"{what}: " + mismatch(a, b))
    tag = f"{form} n={n} {shape} gev={gev} {kind} entry={entry}"
    return [f"{tag}: {x}" for x in msgs], np.asfortranarray(got[PANEL_V][:, m:m + ncorr])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", T1_NS)
def test_dpr_correction_with_m_is_the_applied_block_bit_for_bit(n, form, user):
    n = rows_of(form, n)
    msgs, keep = [], []
    for shape in T1_SHAPES:
        for gev in (False, True):
            with fd.CEngine(n=n, max_cols=shape[0] + shape[1], gev=gev) as e:
                e.cols = cols_alloc(shape[0] + shape[1])
                msgs += dpr_phase(e, n, shape, gev, "wide", "n", form, user, keep)[0]
                msgs += dpr_phase(e, n, shape, gev, "narrow", "g", form, user, keep, m_is_set=True)[0]
    for ctx in keep:
        user.user_op_destroy(ctx)
    assert not msgs, msgs


@pytest.mark.parametrize("form", ["csr", "bsr3", "dia"])
def test_dpr_correction_with_m_has_the_same_bits_on_three_ranks(form):
    n, shape, gev, nranks = 300, (17, 17, 3), True, 3
    with fd.CEngine(n=n, max_cols=shape[0] + shape[1], gev=gev) as e:
        e.cols = cols_alloc(shape[0] + shape[1])
        msgs, t1 = dpr_phase(e, n, shape, gev, "wide", "n", form)
    assert not msgs, msgs

    def work(r, e):
        e.cols = cols_alloc(shape[0] + shape[1])
        return dpr_phase(e, n, shape, gev, "wide", "n", form)
    for msgs, t in run_ranks(nranks, lambda r: fd.CEngine(n=n, max_cols=shape[0] + shape[1], gev=gev, rank=r, nranks=nranks), work):
        assert not msgs, msgs
        assert same_bits(t, t1), mismatch(t, t1)


# ---- T2. the methods that do not read the slot --------------------------------------------------------------------------------------------
def plain_phase(e, m, lowest, v, w, theta, y, method, bv=None):
    """one Ritz phase on the panels: (norms, R, T) - R and T as the panels hold them afterwards, marked beforehand"""
    mark = np.full((v.shape[0], m), 3.25)
    e.panel_put(PANEL_V, m, mark)
    e.panel_put(PANEL_R, 0, mark)
    e.panel_put(PANEL_V, 0, v)
    e.panel_put(PANEL_W, 0, w)
    if bv is not None:
        e.panel_put(PANEL_BV, 0, bv)
    norms = e.ritz_residual_correction(m, lowest, y, theta, method)
    return norms.reshape(1, -1), e.panel_get(PANEL_R, 0, m), e.panel_get(PANEL_V, m, m)


@pytest.mark.parametrize("name,method", [("BDPR", METHOD_BDPR), ("CHEB", METHOD_CHEB), ("LCHEB", METHOD_LCHEB)])
def test_methods_that_do_not_read_m_keep_their_bits(name, method):
    n, m, lowest = 240, 5, 4
    a = BI.block_matrix(n, 4, 1)[0] if name == "BDPR" else P.hamiltonian(12, 20, 0.5, 5)[0]
    v = np.asfortranarray(np.linalg.qr(np.random.default_rng(4).standard_normal((n, m)))[0])
    w = np.asfortranarray(a @ v)
    theta, y = np.linalg.eigh(v.T @ w)
    mm = P.int_banded(n, 9)
    with fd.CEngine(n=n, max_cols=16) as e:
        if name == "BDPR":
            e.set_operator_bsr(OP_A, *P.bsr_of(a, 4))
        else:
            e.set_operator_csr(OP_A, *P.csr_of(a))
        before = plain_phase(e, m, lowest, v, w, theta, y, method)
        dpr_before = plain_phase(e, m, lowest, v, w, theta, y, METHOD_DPR)
        outs = []
        for setter in (lambda: e.set_operator_csr(OP_M, *P.csr_of(mm)), lambda: e.set_operator_bsr(OP_M, *P.bsr_of(mm, 16))):
            setter()
            outs.append(plain_phase(e, m, lowest, v, w, theta, y, method))
        dpr_after = plain_phase(e, m, lowest, v, w, theta, y, METHOD_DPR)
    assert not same_bits(before[2], np.full((n, m), 3.25))               # a correction was written
    for after in outs:
        for what, x, z in zip(("norms", "R", "T"), before, after):
            assert same_bits(x, z), (name, what, mismatch(z, x))
    assert not same_bits(dpr_before[2], dpr_after[2])                    # ... while DPR on the same engine does read the slot


# ---- T3. GJD ------------------------------------------------------------------------------------------------------------------------------
def gjd_solve(e, inp, max_inner, tol):
    e.panel_put(PANEL_V, 0, fenced(inp.n, e.cols, SENTINEL))
    e.panel_put(PANEL_X, 0, inp.x)
    e.panel_put(PANEL_R, 0, inp.r)
    its = e.gjd_correction(inp.m, inp.theta, max_inner, tol)
    return its, e.panel_get(PANEL_V, inp.m, inp.m)


@pytest.mark.parametrize("gev", [False, True])
def test_gjd_with_the_jacobi_diagonal_as_m_restates_the_jacobi_run(gev):
    """One column, M = diag(1 / max(|dA_i - theta dB_i|, 1e-10)) as CSR: r * (1 / k) in place of r / k, one rounding apart per entry.
    The inner tolerance is 1e-6: MINRES amplifies such differences as its Ritz values converge, and near the attainable accuracy the
    step count is no property of the method any more - at 1e-10 the float64 restatement of tests/exact_inputs.py itself stops after
    41 steps with r / k, 22 with r * (1 / k) and 17 in long double (n = 255, standard).  At 1e-6 the restatement takes the same number
    of steps in float64 and in long double (asserted here: a condition on the inputs), and its two float64 variants differ by 1.3e-12
    in T, a hundredth of the bound."""
    n, tol = 1027, 1e-6
    inp = GjdInputs(n, 1, gev, 0)
    steps_64, steps_ld = inp.restate(300, np.float64, tol)[1], inp.restate(300, np.longdouble, tol)[1]
    assert 0 < steps_64 == steps_ld < 300
    with fd.CEngine(n=n, max_cols=4, gev=gev) as e:
        e.cols = cols_alloc(4)
        inp.set_operators(e)
        its_j, t_j = gjd_solve(e, inp, 300, tol)
        kd = np.maximum(np.abs(inp.da - inp.theta[0] * (inp.db if gev else 1.0)), 1e-10)
        e.set_operator_csr(OP_M, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), 1.0 / kd)
        its_m, t_m = gjd_solve(e, inp, 300, tol)
    err = np.abs(t_m - t_j).max() / np.abs(t_j).max()
    print(f"gev={gev}: {its_j} inner steps with the Jacobi diagonal, {its_m} with M = its inverse ({steps_64} in the restatement); "
          f"relative difference of T {err:.3g}")
    assert 0 < its_j < 300 and its_m == its_j
    assert err <= 1e-10


def test_gjd_with_a_dense_inverse_takes_fewer_steps_and_solves_the_equations():
    """the checks of tests/test_solver_gpu.py::test_gjd_correction_solves_the_projected_systems on the Laplacian plus potential, n = 200.
    The basis is the lowest six eigenvectors with noise of 0.01 per entry, orthonormalised: Ritz pairs at the low end of the spectrum,
    as a solve has them (unit vectors at the lowest diagonal entries put theta in the middle of a Laplacian's spectrum, where neither
    preconditioner brings MINRES home in 300 steps).  sigma lies 0.1 below the spectrum, so M = inv(A - sigma I) is positive definite.
    The numpy restatement of the solve takes 106 steps with the Jacobi diagonal and 37 with this M."""
    n, m, lowest = 200, 6, 3
    a = P.hamiltonian(10, 20, 0.5, 21)[0]
    lam_a, vec_a = np.linalg.eigh(a)
    v = np.asfortranarray(np.linalg.qr(vec_a[:, :m] + 0.01 * np.random.default_rng(3).standard_normal((n, m)))[0])
    w = a @ v
    theta, y = np.linalg.eigh(v.T @ w)
    x = v @ y
    r = w @ y - x * theta[None, :]
    sigma = lam_a[0] - 0.1
    minv = np.linalg.inv(a - sigma * np.eye(n))
    minv = 0.5 * (minv + minv.T)

    def run(e):
        e.panel_put(PANEL_V, 0, v)
        e.panel_put(PANEL_W, 0, w)
        e.ritz_residual_correction(m, lowest, y, theta, METHOD_GJD)
        its = e.gjd_correction(m, theta, 300, 1e-10)
        return its, e.panel_get(PANEL_V, m, m)
    with fd.CEngine(n=n, max_cols=2 * m) as e:
        e.set_operator_csr(OP_A, *P.csr_of(a))
        its_j, t_j = run(e)
        e.set_operator_csr(OP_M, *P.csr_of(minv, full=True))
        its_m, t_m = run(e)
    worst = {}
    for name, t in (("Jacobi", t_j), ("M", t_m)):
        worst[name] = 0.0
        for k in range(m):
            proj = np.eye(n) - np.outer(x[:, k], x[:, k])
            res = np.linalg.norm(proj @ (a - theta[k] * np.eye(n)) @ proj @ t[:, k] + r[:, k])
            worst[name] = max(worst[name], res / (1e-8 * max(1.0, np.linalg.norm(r[:, k]))))
    print(f"inner steps: Jacobi {its_j}, M {its_m}; residual of the correction equations / bound: {worst}")
    assert 0 < its_m < its_j
    assert worst["M"] < 1.0


def test_gjd_refuses_an_m_that_is_not_positive_definite():
    n = 255
    inp = GjdInputs(n, 3, False, 0)
    with fd.CEngine(n=n, max_cols=8) as e:
        e.cols = cols_alloc(8)
        inp.set_operators(e)
        e.set_operator_csr(OP_M, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), -np.ones(n))
        basis = fenced(n, e.cols, SENTINEL)
        e.panel_put(PANEL_V, 0, basis)
        e.panel_put(PANEL_X, 0, inp.x)
        e.panel_put(PANEL_R, 0, inp.r)
        with pytest.raises(DavidsonHipError, match=r"preconditioner M \(DAV_OP_M\) is not positive definite"):
            e.gjd_correction(inp.m, inp.theta, 50, 1e-10)
        assert same_bits(e.panel_get(PANEL_V, 0, inp.m), basis[:, :inp.m])
        # the engine is usable: the identity is positive definite
        e.set_operator_identity(OP_M)
        its, t = gjd_solve(e, inp, 50, 1e-10)
        assert its > 0 and np.isfinite(t).all() and t.any()


# ---- T4. solves ---------------------------------------------------------------------------------------------------------------------------
_PLAIN = {}


def set_case(eng, a, b, m=None):
    eng.set_sparse(1, *P.csr_of(a))
    if b is not None:
        eng.set_sparse(2, *P.csr_of(b))
    if m is not None:
        eng.set_sparse(3, *P.csr_of(m, full=True))


def solve(name, method="DPR", with_m=True, policy=None):
    a, b, m, lowest = P.solve_case(name)
    with fd.DavidsonEngine(a.shape[0], lowest, None, gev=b is not None) as eng:
        set_case(eng, a, b, m if with_m else None)
        if policy:
            eng.set_correction_policy(policy)
        return eng.solve(method, P.MAX_ITERATIONS, P.TOLERANCE)


def plain(name, policy=None):
    """the solve without M, once per case and policy"""
    if (name, policy) not in _PLAIN:
        _PLAIN[name, policy] = solve(name, "DPR", False, policy)
    return _PLAIN[name, policy]


def check_solution(name, lam, vec, it):
    a, b, _, lowest = P.solve_case(name)
    assert it <= P.MAX_ITERATIONS
    assert np.abs(lam - P.eigh_lowest(a, b, lowest)).max() < 1e-9
    assert (P.residual_norms(a, b, lam, vec) < P.TOLERANCE).all()


@pytest.mark.parametrize("name", list(P.SOLVE_CASES))
def test_dpr_solve_with_m_needs_at_most_half_the_iterations(name):
    lam0, vec0, it0 = plain(name)
    lam, vec, it = solve(name)
    print(f"{name}: plain DPR {it0} iterations, with M {it}")
    check_solution(name, lam0, vec0, it0)
    check_solution(name, lam, vec, it)
    assert 2 * it <= it0, (it, it0)


def test_gjd_solve_of_the_generalized_pencil_with_m():
    lam, vec, it = solve("n400_gev", "GJD")
    lam0, vec0, it0 = solve("n400_gev", "GJD", with_m=False)
    print(f"n400_gev GJD: {it0} outer iterations with the Jacobi diagonal, {it} with M")
    check_solution("n400_gev", lam, vec, it)
    check_solution("n400_gev", lam0, vec0, it0)


@pytest.mark.parametrize("policy", ["unconverged", "locking"])
def test_dpr_solve_with_m_under_the_other_policies(policy):
    lam0, vec0, it0 = plain("n400_std", policy)
    lam, vec, it = solve("n400_std", policy=policy)
    print(f"n400_std, policy {policy}: plain DPR {it0} iterations, with M {it}")
    check_solution("n400_std", lam, vec, it)
    assert it < it0, (it, it0)


def solve_on_ranks(nranks, n, lowest, gev, setup):
    """the solve on nranks local-group ranks (threads of this process, as tests/test_device_operator_gpu.py): [(lam, vec, it)] per rank"""
    engs = [fd.DavidsonEngine(n, lowest, None, gev=gev, rank=r, nranks=nranks) for r in range(nranks)]
    handles = (C.c_void_p * nranks)(*[e.c.h for e in engs])
    assert fd.hip_lib().dav_local_group_join(handles, nranks) == 0
    out, err = [None] * nranks, [None] * nranks

    def work(r):
        try:
            setup(engs[r])
            out[r] = engs[r].solve("DPR", P.MAX_ITERATIONS, P.TOLERANCE)
        except Exception as exc:      # noqa: BLE001
            err[r] = exc
        finally:
            fd.hip_lib().dav_local_group_yield(engs[r].c.h)
    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join() for t in th]
    for e in engs:
        e.close()
    assert all(x is None for x in err), err
    return out


def test_dpr_solve_with_m_on_three_ranks_counts_as_on_one():
    a, b, m, lowest = P.solve_case("n400_std")
    lam1, _, it1 = solve("n400_std")
    for lam, vec, it in solve_on_ranks(3, a.shape[0], lowest, False, lambda eng: set_case(eng, a, b, m)):
        assert it == it1, (it, it1)
        assert np.abs(lam - lam1).max() < 1e-12
        check_solution("n400_std", lam, vec, it)


def test_whether_m_is_set_is_one_of_the_inputs_the_ranks_agree_on():
    """dav_agree_inputs (what the driver calls before a solve): ranks that all have M, or all lack it, pass - and setting M on every rank
    is a change of the inputs, verified again; a rank that differs is an error ON EVERY RANK, as for the driver's own words (the cases
    of tests/test_kernels_gpu.py::test_solve_inputs_are_verified_in_a_fixed_size_collective_when_they_change)"""
    nranks, n = 3, 300
    words = [300.0, 3.0, 30.0, 100.0, 1e-8, 0.0, 0.0, 1.0, 0.0, 0.0]
    mm = P.csr_of(P.int_banded(n, 2))

    def work(r, e):
        e.reset_stats()
        e.agree_inputs(words)
        e.agree_inputs(words)
        assert e.stats().collectives == 1
        e.set_operator_csr(OP_M, *mm)
        e.agree_inputs(words)
        assert e.stats().collectives == 2                        # every rank set M: verified again, and agreed
        e.agree_inputs(words)
        assert e.stats().collectives == 2
        return "agreed"
    out = run_ranks(nranks, lambda r: fd.CEngine(n=n, max_cols=16, rank=r, nranks=nranks), work)
    assert all(o == "agreed" for o in out), out

    def lone(r, e):
        if r == 1:
            e.set_operator_csr(OP_M, *mm)
        try:
            e.agree_inputs(words)
        except DavidsonHipError as exc:
            return str(exc)
        return "no error"
    out = run_ranks(nranks, lambda r: fd.CEngine(n=n, max_cols=16, rank=r, nranks=nranks), lone)
    assert all("ranks disagree" in o and "word 10" in o for o in out), out


def test_the_stencil_as_a_device_callback_solves_as_the_same_matrix_as_csr(user):
    a, b, _, lowest = P.solve_case("n400_std")
    n = a.shape[0]
    ms = P.stencil_matrix(n, 1.0, 0.0, 0.2)                 # symmetric positive definite: 1 - 0.6 <= its eigenvalues
    ctx = user.user_op_create(1.0, 0.0, 0.2)
    out = []
    for how in ("csr", "callback"):
        with fd.DavidsonEngine(n, lowest, None) as eng:
            set_case(eng, a, b)
            if how == "csr":
                eng.set_sparse(3, *P.csr_of(ms))
            else:
                eng.set_device_operator(3, user.user_op_apply, ctx, diag=None)
            out.append(eng.solve("DPR", P.MAX_ITERATIONS, P.TOLERANCE))
    user.user_op_destroy(ctx)
    (lam_c, vec_c, it_c), (lam_d, vec_d, it_d) = out
    print(f"stencil M: {it_c} iterations as CSR, {it_d} as a callback")
    assert it_c == it_d
    assert np.abs(lam_c - lam_d).max() < 1e-12
    check_solution("n400_std", lam_d, vec_d, it_d)


# ---- T5. new values of M --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["csr", "dia", "bsr3"])
def test_new_values_on_the_kept_pattern_of_m_give_the_t_of_a_fresh_set_call(form):
    n, m, lowest = 300, 5, 4
    rng = np.random.default_rng(_seed("refresh", form))
    a = P.hamiltonian(15, 20, 0.5, 6)[0]
    v = np.asfortranarray(np.linalg.qr(rng.standard_normal((n, m)))[0])
    w = np.asfortranarray(a @ v)
    theta, y = np.linalg.eigh(v.T @ w)
    m1 = P.int_banded(n, 1).astype(np.float64)
    m2 = np.where(m1 != 0.0, m1 + 0.25, 0.0)              # the same pattern, other numbers

    def arrays(mat):
        return P.bsr_of(mat, 3) if form == "bsr3" else P.csr_of(mat)

    def set_form(e, mat):
        if form == "bsr3":
            e.set_operator_bsr(OP_M, *arrays(mat))
        else:
            e.set_operator_csr(OP_M, *arrays(mat), diagonals=form == "dia")

    with fd.CEngine(n=n, max_cols=16) as e:
        e.set_operator_csr(OP_A, *P.csr_of(a))
        e.keep_value_map(OP_M)
        set_form(e, m1)
        first = plain_phase(e, m, lowest, v, w, theta, y, METHOD_DPR)
        e.update_operator_values(OP_M, arrays(m2)[2])
        updated = plain_phase(e, m, lowest, v, w, theta, y, METHOD_DPR)
        diag = e.get_diagonal(OP_M)
    with fd.CEngine(n=n, max_cols=16) as e:
        e.set_operator_csr(OP_A, *P.csr_of(a))
        set_form(e, m2)
        fresh = plain_phase(e, m, lowest, v, w, theta, y, METHOD_DPR)
    assert not same_bits(first[2], updated[2])
    for what, x, z in zip(("norms", "R", "T"), updated, fresh):
        assert same_bits(x, z), (what, mismatch(x, z))
    assert np.allclose(updated[2], m2 @ updated[1], rtol=0, atol=1e-13 * np.abs(m2 @ updated[1]).max())
    assert np.array_equal(diag, np.diag(m2))


# ---- T6. the C entries that refuse the slot ---------------------------------------------------------------------------------------------------
def test_the_entries_that_serve_a_and_b_only_name_the_slot_and_leave_the_engine_usable(tmp_path):
    a, b, m, lowest = P.solve_case("n400_std")
    n = a.shape[0]
    with fd.DavidsonEngine(n, lowest, None) as eng:
        e = eng.c
        set_case(eng, a, b, m)
        refused = {
            "dav_set_dense_host": lambda: e.set_dense_host(OP_M, np.eye(n)),
            "dav_set_dense_dev": lambda: e.set_dense_dev(OP_M, None, n),
            "dav_dense_begin": lambda: e.dense_begin(OP_M),
            "dav_dense_put_rows": lambda: e.dense_put_rows(OP_M, 0, np.ones((1, n))),
            "dav_dense_end": lambda: e.dense_end(OP_M),
            "dav_set_dense_file": lambda: e.set_dense_file(OP_M, tmp_path / "no_such_file.txt"),
            "dav_set_dense_generated": lambda: e.set_dense_generated(OP_M, 1, 1e-2),
            "dav_set_operator_hashed": lambda: e.set_operator_hashed(OP_M, 1, 1e-2),
            "dav_set_operator_harness": lambda: e.set_operator_harness(OP_M, np.ones(n)),
            "dav_set_operator_host": lambda: e.set_operator_host(OP_M, np.ones(n)),
        }
        for name, call in refused.items():
            with pytest.raises(DavidsonHipError, match="DAV_OP_M"):
                call()
        for call in (lambda: e.apply(3, PANEL_V, 0, 1, PANEL_W, 0), lambda: e.set_operator_identity(3), lambda: e.keep_value_map(3),
                     lambda: e.set_operator_csr(3, *P.csr_of(np.eye(n)))):
            with pytest.raises(DavidsonHipError, match="bad operator id"):
                call()
        # the slot still holds the M set before the refusals: it applies and the solve counts as in T4
        x = np.asfortranarray(np.random.default_rng(1).standard_normal((n, 3)))
        e.panel_put(PANEL_V, 0, x)
        e.apply(OP_M, PANEL_V, 0, 3, PANEL_W, 0)
        assert np.allclose(e.panel_get(PANEL_W, 0, 3), m @ x, rtol=0, atol=1e-12 * np.abs(m @ x).max())
        lam, vec, it = eng.solve("DPR", P.MAX_ITERATIONS, P.TOLERANCE)
    check_solution("n400_std", lam, vec, it)
    assert 2 * it <= plain("n400_std")[2]
