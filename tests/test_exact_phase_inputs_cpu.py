"""CPU: the references of tests/test_exact_phases_gpu.py are what that module takes them for - the integer inputs of parts A - C keep
every partial sum below 2^53 (so any order of summation is exact), the dyadic DPR block is exact, the float64 restatement of the GJD
correction lies within gamma(n) of the long-double one on every part D case, and the restatement solves the projected systems."""
import numpy as np
import pytest

from exact_inputs import (dpr_diagonals, dpr_reference, gamma, gjd_restatement, int_block, int_matrix, int_product, ritz_inputs,
                          ritz_reference, tridiag_csr, tridiag_mul, unit_block)
from oracle import davidson_oracle as O
from test_exact_phases_gpu import (GJD_MS, GJD_NS, GJD_SPECIAL, GJD_STEPS, ORTHO_APPLY_SHAPES, RESTART_SHAPES, RITZ_LARGE, RITZ_NS,
                                   RITZ_SHAPES, gjd_all_cases, gjd_references)

LIMIT = 2.0 ** 53


def _abs_sum(p, m):
    """the largest sum of |terms| of any entry of P M: a bound of every partial sum in any order"""
    return float(np.max(np.abs(p) @ np.abs(m))) if p.size and m.size else 0.0


@pytest.mark.parametrize("kind", ["wide", "narrow"])
@pytest.mark.parametrize("gev", [False, True])
def test_ritz_inputs_keep_every_partial_sum_exact(kind, gev):
    rng = np.random.default_rng(7)
    for n, (m, ncorr, lowest) in [(n, s) for n in RITZ_NS for s in RITZ_SHAPES] + RITZ_LARGE:
        for dyadic in (False, True):
            v, w, z, y, theta = ritz_inputs(kind, n, m, ncorr, gev, rng, dyadic)
            assert np.all(theta == np.round(theta)) and np.all(np.abs(theta) >= 1)
            y2 = -y * theta[None, :]                                       # what the host builds
            assert np.array_equal(y2, -(y.astype(np.int64) * theta.astype(np.int64)[None, :]))
            xi, ri, ss = ritz_reference(v, w, z, y, theta)
            assert _abs_sum(v, y) < LIMIT and _abs_sum(w, y) + _abs_sum(z, y2) < LIMIT
            if kind == "wide":
                assert np.abs(v).max(initial=0) < 2 ** 20 and np.abs(y).max() <= 7 and np.abs(theta).max() <= 8
                assert np.abs(xi).max() < 2 ** 30 and np.abs(ri).max() < 2 ** 33
            else:
                assert np.abs(y).max() <= 3 and np.abs(theta).max() <= 2
                assert np.abs(ri).max() <= 1152 and n < 2 ** 14 and ss.max() < 2 ** 36
                # the squared norms are exact in float64 in any order, so sqrt of the integer is what the host must return
                assert np.array_equal(np.sum(ri.astype(np.float64) ** 2, axis=0), ss.astype(np.float64))
            # float64 products of these inputs are the int64 ones: nothing is lost in any order
            assert np.array_equal(w @ y + z @ y2, ri.astype(np.float64))
            if dyadic:
                da, db, _ = dpr_diagonals(n, gev, theta, rng, None)
                t, den = dpr_reference(ri, theta, da, db)
                k = np.log2(np.abs(den))
                assert np.all(k == np.round(k)) and k.max() <= 5 and k.min() >= 0
                assert np.array_equal(t * den, ri.astype(np.float64)) and np.array_equal(t * 32, np.round(t * 32))
                if kind == "narrow":
                    assert np.sum((t * 32) ** 2, axis=0).max() < 2 ** 46                 # T^T T and V^T T are exact
                    assert np.array_equal(v.T @ t, (v.astype(np.int64).T @ (t * 32).astype(np.int64)) / 32.0)
            else:
                da, db, rows = dpr_diagonals(n, gev, theta, rng, lowest - 1)
                t, den = dpr_reference(ri, theta, da, db)
                assert np.abs(da).max() <= 40 and rows.size and {0, n - 1} <= set(rows.tolist())
                assert (den[rows, lowest - 1] == 0).all() and (t[rows, lowest - 1] == 0).all()
                assert n < 129 or ({127, 128} & set(rows.tolist()))


def test_ortho_and_restart_inputs_keep_every_partial_sum_exact():
    rng = np.random.default_rng(11)
    n = 2305
    for m, kt in ORTHO_APPLY_SHAPES:
        v, lead, t = unit_block(n, m, rng), int_block(n, m, rng, bits=20), int_block(n, kt, rng, bits=20)
        c, mm = int_matrix(m, kt, rng), int_matrix(kt, kt, rng)
        cm = -int_product(c, mm)
        host = np.zeros((m, kt))
        for j in range(kt):                                                # the host's -(C M), term by term in float64
            for l in range(kt):
                host[:, j] -= c[:, l] * mm[l, j]
        assert np.array_equal(host, cm.astype(np.float64))
        assert _abs_sum(t, mm) + _abs_sum(lead, cm.astype(np.float64)) < LIMIT
        assert _abs_sum(t.T, t) < LIMIT and _abs_sum(v.T, t) < LIMIT and _abs_sum(lead.T, t) < LIMIT       # the Gram blocks
    for m, keep in RESTART_SHAPES:
        assert _abs_sum(int_block(n, m, rng, bits=20), int_matrix(m, keep, rng)) < 2 ** 30


def test_tridiagonal_csr_is_the_matrix_the_restatement_multiplies_by():
    rng = np.random.default_rng(3)
    n = 37
    d, off, v = rng.random(n), rng.standard_normal(n - 1), rng.standard_normal((n, 3))
    indptr, indices, data = tridiag_csr(d, off)
    a = np.zeros((n, n))
    for i in range(n):
        a[i, indices[indptr[i]:indptr[i + 1]]] = data[indptr[i]:indptr[i + 1]]
    assert np.array_equal(a, np.diag(d) + np.diag(off, 1) + np.diag(off, -1))
    assert np.allclose(tridiag_mul(d, off, v), a @ v, rtol=0, atol=1e-14)


def test_every_gjd_case_is_inside_the_condition_of_its_bar():
    """the float64 run of the restatement lies within gamma(n) of the long-double run, so 8 gamma(n) asks the engine for no more than
    the reference itself delivers"""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    cases = gjd_all_cases()
    assert len(cases) == len(GJD_NS) * len(GJD_MS) * 2 * len(GJD_STEPS) + sum(len(c[4]) for c in GJD_SPECIAL.values())
    worst = 0.0
    for n, m, gev, steps, kw in cases:
        inp, t_ld, err64 = gjd_references(n, m, gev, steps, **kw)
        assert np.isfinite(t_ld.astype(np.float64)).all()
        assert err64 <= gamma(n), (n, m, gev, steps, kw, err64 / gamma(n))
        worst = max(worst, err64 / gamma(n))
    print(f"float64 restatement against long double: worst error / gamma(n) = {worst:.3f}")


def test_the_floor_case_reaches_the_floor_and_is_ill_conditioned_from_two_steps_on():
    n, _, m, gev, _, kw = GJD_SPECIAL["floor"]
    inp, _, _ = gjd_references(n, m, gev, 1, **kw)
    i0 = n // 2
    assert inp.da[i0] - inp.theta[0] * 1.0 == 0.0 and not inp.x[i0].any() and inp.r[i0, 0] == 2.0 ** -40
    t1, _ = inp.restate(1, np.float64)
    assert abs(t1[i0, 0]) > 1e3 * 2.0 ** -40               # K^-1 carries 1e10 there


def test_the_restatement_solves_the_projected_systems():
    """the comparison of test_solver_gpu.py::test_gjd_correction_solves_the_projected_systems, with the restatement for the engine"""
    n, m = 300, 6
    a = O.generate_diagonal_dominant(n, 1e-2, seed=8)
    v = O.generate_preconditioner(np.diag(a).copy(), m)
    w = a @ v
    theta, y = O.lapack_generalized_eigensolver(v.T @ w)
    x = v @ y
    r = w @ y - x * theta[None, :]
    t_ref = O.compute_GJD_generalized_dense(a, theta, x, r)
    t, its = gjd_restatement(lambda u: a @ u, None, np.diag(a).copy(), None, x, r, theta, 300, np.float64, 1e-10)
    assert 0 < its < 300
    for k in range(m):
        p = np.eye(n) - np.outer(x[:, k], x[:, k])
        mk = p @ (a - theta[k] * np.eye(n)) @ p
        assert np.linalg.norm(mk @ t[:, k] + r[:, k]) < 1e-8 * max(1.0, np.linalg.norm(r[:, k]))
        assert np.linalg.norm(p @ t[:, k] - p @ t_ref[:, k]) < 1e-6 * max(1e-30, np.linalg.norm(p @ t_ref[:, k]))
