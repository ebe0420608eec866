!> The Chebyshev-filtered correction as a Fortran user sees it: methods "CHEB" and "CHEB16" of the generic generalized_eigensolver on a
!> csr_matrix and on a bsr_matrix.  The 5-point Laplacian of a 16 x 16 grid with a slightly perturbed diagonal from an integer formula
!> (the test rebuilds it in numpy) - the kind of matrix on which scalar "DPR" is slow because its diagonal is nearly constant -, solved
!> with the default degree in both forms, with degree 16, and once with "DPR" for the iteration count.  Prints "CHECK name T|F" lines,
!> the eigenvalues and the iteration counts, and stops with a non-zero code on any F.
program prog_cheb
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, csr_matrix, bsr_matrix
  implicit none
  integer, parameter :: nx = 16, n = nx * nx, lowest = 4, bs = 4, nb = n / bs
  real(dp) :: dense(n, n)
  type(csr_matrix) :: a
  type(bsr_matrix) :: ab
  real(dp) :: ev(lowest), ev_bsr(lowest), ev_16(lowest), ev_dpr(lowest)
  real(dp) :: x(n, lowest), x_bsr(n, lowest), x_16(n, lowest), x_dpr(n, lowest)
  integer :: it, it_bsr, it_16, it_dpr, j, nfail

  nfail = 0
  call laplacian(dense)
  a = as_csr(dense)
  ab = as_bsr(dense)

  call generalized_eigensolver(a, ev, x, lowest, "CHEB", 400, 1d-8, it)
  call generalized_eigensolver(ab, ev_bsr, x_bsr, lowest, "CHEB", 400, 1d-8, it_bsr)
  call generalized_eigensolver(a, ev_16, x_16, lowest, "CHEB16", 400, 1d-8, it_16)
  call generalized_eigensolver(a, ev_dpr, x_dpr, lowest, "DPR", 400, 1d-8, it_dpr)

  do j = 1, lowest
     call check("residual_csr", norm2(matmul(dense, x(:, j)) - ev(j) * x(:, j)) < 1d-8)
     call check("residual_bsr", norm2(matmul(dense, x_bsr(:, j)) - ev_bsr(j) * x_bsr(:, j)) < 1d-8)
     call check("residual_d16", norm2(matmul(dense, x_16(:, j)) - ev_16(j) * x_16(:, j)) < 1d-8)
  end do
  print "(a, 4i6)", "ITERS", it, it_bsr, it_16, it_dpr
  print "(a, 4es26.17)", "EVALS_CSR", ev
  print "(a, 4es26.17)", "EVALS_BSR", ev_bsr
  print "(a, 4es26.17)", "EVALS_D16", ev_16
  if (nfail > 0) error stop 1

contains

  subroutine laplacian(m)
    real(dp), intent(out) :: m(n, n)
    integer :: i, j, p
    m = 0.0_dp
    do i = 1, nx
       do j = 1, nx
          p = (i - 1) * nx + j
          m(p, p) = 4.0_dp + 0.05_dp * (real(mod(37 * p + 11, 101), dp) / 101.0_dp - 0.5_dp)
          if (j < nx) then
             m(p, p + 1) = -1.0_dp
             m(p + 1, p) = -1.0_dp
          end if
          if (i < nx) then
             m(p, p + nx) = -1.0_dp
             m(p + nx, p) = -1.0_dp
          end if
       end do
    end do
  end subroutine laplacian

  function as_csr(m) result(c)
    real(dp), intent(in) :: m(n, n)
    type(csr_matrix) :: c
    integer :: row_ptr(n + 1), col_idx(5 * n), i, j, nnz
    real(dp) :: vals(5 * n)
    nnz = 0
    do i = 1, n
       row_ptr(i) = nnz + 1
       do j = 1, n
          if (m(i, j) /= 0.0_dp) then
             nnz = nnz + 1
             col_idx(nnz) = j
             vals(nnz) = m(i, j)
          end if
       end do
    end do
    row_ptr(n + 1) = nnz + 1
    c = csr_matrix(n, row_ptr, col_idx(1:nnz), vals(1:nnz), .false.)
  end function as_csr

  function as_bsr(m) result(c)
    real(dp), intent(in) :: m(n, n)
    type(bsr_matrix) :: c
    integer :: row_ptr(nb + 1), col_idx(5 * nb), bi, bj, nnzb
    real(dp) :: vals(bs, bs, 5 * nb)
    nnzb = 0
    do bi = 1, nb
       row_ptr(bi) = nnzb + 1
       do bj = 1, nb
          if (any(m((bi - 1) * bs + 1 : bi * bs, (bj - 1) * bs + 1 : bj * bs) /= 0.0_dp)) then
             nnzb = nnzb + 1
             col_idx(nnzb) = bj
             vals(:, :, nnzb) = m((bi - 1) * bs + 1 : bi * bs, (bj - 1) * bs + 1 : bj * bs)
          end if
       end do
    end do
    row_ptr(nb + 1) = nnzb + 1
    c = bsr_matrix(n, bs, row_ptr, col_idx(1:nnzb), vals(:, :, 1:nnzb), .false.)
  end function as_bsr

  subroutine check(name, ok)
    character(len=*), intent(in) :: name
    logical, intent(in) :: ok
    print "(a, 1x, a, 1x, l1)", "CHECK", name, ok
    if (.not. ok) nfail = nfail + 1
  end subroutine check

end program prog_cheb
