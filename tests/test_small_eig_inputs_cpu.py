"""The reference of tests/test_small_eig_spectra_gpu.py checked against itself: on every input family LAPACK (what the GPU
test compares the kernel with) must sit well inside the tolerances that test grants the kernel - against 50-digit
arithmetic (mpmath) at small orders, through its own residual and orthogonality at the large ones.  A family that fails
here is a bad family, not a reason for a wider tolerance."""
import mpmath
import numpy as np
import pytest
import scipy.linalg

import small_eig_inputs as F

EV_TOL, ORTH_TOL, RES_TOL, GRADED_REL_TOL = 1e-12, 1e-12, 1e-13, 1e-11      # what the GPU test grants the kernel
MARGIN = 10.0                                                                # LAPACK sits this far inside
SOLVABLE = {**F.STANDARD, **F.GENERALIZED}


def mp_eigenvalues(H, S, digits=50):
    """ascending eigenvalues of H y = theta S y in `digits`-digit arithmetic, as mpmath numbers"""
    with mpmath.workdps(digits):
        A = mpmath.matrix(H.tolist())
        if S is not None:
            L = mpmath.cholesky(mpmath.matrix(S.tolist()))
            Li = mpmath.inverse(L)
            A = Li * A * Li.T
            A = (A + A.T) / 2
        ev = mpmath.eigsy(A, eigvals_only=True)
        return sorted(ev[i] for i in range(len(ev)))


@pytest.mark.parametrize("m", [1, 2, 3, 8, 33, 128])
@pytest.mark.parametrize("name", sorted(F.FAMILIES))
def test_inputs_are_exactly_symmetric_and_reproducible(name, m):
    H, S = F.FAMILIES[name](m, 0)
    H2, S2 = F.FAMILIES[name](m, 0)
    for X, X2 in ((H, H2), (S, S2)):
        if X is None:
            continue
        assert X.shape == (m, m) and X.dtype == np.float64
        assert np.array_equal(X, X.T) and np.array_equal(X, X2) and np.isfinite(X).all()


@pytest.mark.parametrize("m", [5, 16, 24])
@pytest.mark.parametrize("name", sorted(SOLVABLE))
def test_lapack_against_50_digits(name, m):
    H, S = SOLVABLE[name](m, 0)
    ref = scipy.linalg.eigh(H, S, eigvals_only=True)
    exact = mp_eigenvalues(H, S)
    err = np.array([float(abs(mpmath.mpf(float(r)) - x)) for r, x in zip(ref, exact)])
    scale = max(float(abs(x)) for x in exact)
    if name == "S_cond1e10":
        # LAPACK is NOT accurate to 1e-12 of the largest eigenvalue here (about 1e-7 at order 5).  The reduced matrix
        # C = L^-1 H L^-T comes out of two triangular solves of condition cond(L)^2 = cond(S), so it carries a forward error
        # of eps cond(S) ||C||, and by Weyl every eigenvalue moves by at most that: eps cond(S) max|theta|.  LAPACK alone
        # sits ten times inside; the GPU test grants the device and LAPACK together ten times the bound
        assert err.max() <= 2.0 ** -52 * np.linalg.cond(S) * scale / MARGIN, err.max() / scale
        assert err.max() > EV_TOL * scale or m > 5          # the reason this family has a bound of its own
        return
    assert err.max() <= EV_TOL / MARGIN * scale, (err.max(), scale)
    if name == "graded_scaled":
        # the entries determine every eigenvalue to high relative accuracy, and the 50-digit values have it: they are the
        # reference of the relative test (LAPACK is only asked for norm-wise accuracy on this family)
        lo = mp_eigenvalues(H, S, digits=30)
        assert max(float(abs(a - b) / abs(b)) for a, b in zip(lo, exact)) <= 1e-20
        assert min(float(x) for x in exact) > 0.0


@pytest.mark.parametrize("m", [33, 64, 98, 128])
@pytest.mark.parametrize("name", sorted(SOLVABLE))
def test_lapack_residual_and_orthogonality_at_the_large_orders(name, m):
    H, S = SOLVABLE[name](m, 0)
    # DSYEVD / DSYGVD, what the host path of the solver calls (the default driver, DSYEVR, gives up orthogonality - 2e-13 at
    # order 98 - on the tight pairs of wilkinson and the like)
    theta, Y = scipy.linalg.eigh(H, S, driver="evd" if S is None else "gvd")
    if name == "S_cond1e10":
        # no bound is owed here (the Cholesky reduction loses cond(S) eps); the GPU test measures LAPACK on the same input
        # and grants the kernel ten times that.  What must hold: the input is as ill-conditioned as it says, and LAPACK works
        assert 1e9 <= np.linalg.cond(S) <= 1e11 and np.isfinite(theta).all()
        return
    assert F.scaled_residual(H, S, theta, Y) <= RES_TOL / MARGIN
    assert F.orthogonality(S, Y) <= ORTH_TOL / MARGIN


@pytest.mark.parametrize("m", [3, 8, 33, 64, 98, 128])
def test_not_positive_definite_overlaps_fail_at_the_stated_pivot(m):
    """the first non-positive pivot of a right-looking Cholesky, counted from 1"""
    def first_bad_pivot(S):
        A = S.copy()
        for j in range(len(A)):
            if not A[j, j] > 0.0:
                return j + 1
            A[j + 1:, j] /= np.sqrt(A[j, j])
            A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
        return 0
    assert first_bad_pivot(F.S_late_negative(m)[1]) == m
    assert first_bad_pivot(F.S_semidefinite(m)[1]) == m // 2 + 1
    assert first_bad_pivot(F.S_near_identity(m)[1]) == 0 and first_bad_pivot(F.S_cond1e10(m)[1]) == 0


def test_structure_of_the_special_families():
    m = 33
    H = F.diagonal(m)[0]
    assert np.count_nonzero(H - np.diag(np.diag(H))) == 0 and (np.diff(np.diag(H)) < 0).any()      # diagonal, not sorted
    ev = np.linalg.eigvalsh(F.two_values(m)[0])
    assert np.abs(ev[:17] + 2.0).max() < 1e-13 and np.abs(ev[17:] - 1.0).max() < 1e-13
    ev = np.linalg.eigvalsh(F.cluster(m)[0])
    assert np.abs(ev[:16] - 1.0).max() < 1e-11 and np.allclose(ev[16:], 2.0 + np.arange(17))
    assert np.linalg.matrix_rank(F.rank_one(m)[0]) == 1
    ev = np.linalg.eigvalsh(F.null_space(m)[0])
    assert np.abs(ev[:3]).max() < 1e-13 and np.allclose(ev[3:], np.arange(1.0, 31.0))
    assert np.abs(F.scaled_down(m)[0]).max() < 1e-99 and np.abs(F.scaled_up(m)[0]).max() > 1e99
