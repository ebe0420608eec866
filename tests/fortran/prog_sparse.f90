!> Sparse path as a Fortran user sees it: a banded symmetric matrix built as a csr_matrix (1-based, default-kind integers), solved
!> through the generic generalized_eigensolver of module davidson - standard (DPR, GJD) and generalized with a banded B, and once
!> more from the lower triangle only.  Prints "CHECK name T|F" lines, the eigenvalues and iteration counts, and stops with a
!> non-zero code on any F.
program prog_sparse
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, csr_matrix
  implicit none
  integer, parameter :: n = 1200, lowest = 4
  type(csr_matrix) :: a, b, a_low
  real(dp) :: ev(lowest), ev_gjd(lowest), ev_gen(lowest), ev_low(lowest)
  real(dp) :: x(n, lowest), x_gjd(n, lowest), x_gen(n, lowest), x_low(n, lowest)
  integer :: it, it_gjd, it_gen, it_low, j, nfail

  nfail = 0
  a = banded(1.0_dp, 1.0_dp, 0.3_dp, .false.)
  a_low = banded(1.0_dp, 1.0_dp, 0.3_dp, .true.)
  b = banded(1.0_dp, 0.0_dp, 0.05_dp, .false.)

  call generalized_eigensolver(a, ev, x, lowest, "DPR", 1000, 1d-8, it)
  call generalized_eigensolver(a, ev_gjd, x_gjd, lowest, "GJD", 1000, 1d-8, it_gjd)
  call generalized_eigensolver(a, ev_gen, x_gen, lowest, "DPR", 1000, 1d-8, it_gen, 10 * lowest, b)
  call generalized_eigensolver(a_low, ev_low, x_low, lowest, "DPR", 1000, 1d-8, it_low)

  call check("gjd_equals_dpr", maxval(abs(ev_gjd - ev)) < 1d-8)
  call check("lower_equals_full", maxval(abs(ev_low - ev)) < 1d-12 .and. it_low == it)
  do j = 1, lowest
     call check("residual_dpr", norm2(spmv(a, x(:, j)) - ev(j) * x(:, j)) < 1d-8)
     call check("residual_gjd", norm2(spmv(a, x_gjd(:, j)) - ev_gjd(j) * x_gjd(:, j)) < 1d-8)
     call check("residual_gen", norm2(spmv(a, x_gen(:, j)) - ev_gen(j) * spmv(b, x_gen(:, j))) < 1d-8)
  end do
  print "(a, 4i6)", "ITERS", it, it_gjd, it_gen, it_low
  print "(a, 4es26.17)", "EVALS_DPR", ev
  print "(a, 4es26.17)", "EVALS_GJD", ev_gjd
  print "(a, 4es26.17)", "EVALS_GEN", ev_gen
  if (nfail > 0) error stop 1

contains

  !> d0 + dstep * (i - 1) on the diagonal, eps on the first and eps / 2 on the second off-diagonals; lower = only j <= i
  function banded(d0, dstep, eps, lower) result(m)
    real(dp), intent(in) :: d0, dstep, eps
    logical, intent(in) :: lower
    type(csr_matrix) :: m
    integer :: row_ptr(n + 1), col_idx(5 * n), i, j, nnz
    real(dp) :: vals(5 * n)
    nnz = 0
    do i = 1, n
       row_ptr(i) = nnz + 1
       do j = max(1, i - 2), merge(i, min(n, i + 2), lower)
          nnz = nnz + 1
          col_idx(nnz) = j
          select case (abs(i - j))
          case (0)
             vals(nnz) = d0 + dstep * real(i - 1, dp)
          case (1)
             vals(nnz) = eps
          case default
             vals(nnz) = 0.5_dp * eps
          end select
       end do
    end do
    row_ptr(n + 1) = nnz + 1
    m = csr_matrix(n, row_ptr, col_idx(1:nnz), vals(1:nnz), lower)
  end function banded

  function spmv(m, v) result(y)
    type(csr_matrix), intent(in) :: m
    real(dp), intent(in) :: v(:)
    real(dp) :: y(size(v))
    integer :: i
    integer(8) :: p
    y = 0.0_dp
    do i = 1, m%n
       do p = m%row_ptr(i), m%row_ptr(i + 1) - 1
          y(i) = y(i) + m%values(p) * v(m%col_idx(p))
       end do
    end do
  end function spmv

  subroutine check(name, ok)
    character(len=*), intent(in) :: name
    logical, intent(in) :: ok
    print "(a, 1x, a, 1x, l1)", "CHECK", name, ok
    if (.not. ok) nfail = nfail + 1
  end subroutine check

end program prog_sparse
