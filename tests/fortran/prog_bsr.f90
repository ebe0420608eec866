!> Block-sparse path as a Fortran user sees it: a banded symmetric matrix built as a bsr_matrix with 4 x 4 blocks (1-based, default-kind
!> integers, values(b, b, nnzb)), solved through the generic generalized_eigensolver of module davidson - standard (DPR, GJD) and
!> generalized with a banded B, and once more from the lower block triangle only.  Prints "CHECK name T|F" lines, the eigenvalues and
!> iteration counts, and stops with a non-zero code on any F.
program prog_bsr
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, bsr_matrix
  implicit none
  integer, parameter :: n = 1200, lowest = 4, bs = 4, nb = n / bs
  type(bsr_matrix) :: a, b, a_low
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
     call check("residual_dpr", norm2(bsrmv(a, x(:, j)) - ev(j) * x(:, j)) < 1d-8)
     call check("residual_gjd", norm2(bsrmv(a, x_gjd(:, j)) - ev_gjd(j) * x_gjd(:, j)) < 1d-8)
     call check("residual_gen", norm2(bsrmv(a, x_gen(:, j)) - ev_gen(j) * bsrmv(b, x_gen(:, j))) < 1d-8)
  end do
  print "(a, 4i6)", "ITERS", it, it_gjd, it_gen, it_low
  print "(a, 4es26.17)", "EVALS_DPR", ev
  print "(a, 4es26.17)", "EVALS_GJD", ev_gjd
  print "(a, 4es26.17)", "EVALS_GEN", ev_gen
  if (nfail > 0) error stop 1

contains

  !> entry (i, j) of the band: d0 + dstep * (i - 1) on the diagonal, eps on the first and eps / 2 on the second off-diagonals
  pure real(dp) function entry(i, j, d0, dstep, eps)
    integer, intent(in) :: i, j
    real(dp), intent(in) :: d0, dstep, eps
    select case (abs(i - j))
    case (0)
       entry = d0 + dstep * real(i - 1, dp)
    case (1)
       entry = eps
    case (2)
       entry = 0.5_dp * eps
    case default
       entry = 0.0_dp
    end select
  end function entry

  !> the band as block-tridiagonal 4 x 4 blocks; lower = only the blocks with block column <= block row
  function banded(d0, dstep, eps, lower) result(m)
    real(dp), intent(in) :: d0, dstep, eps
    logical, intent(in) :: lower
    type(bsr_matrix) :: m
    integer :: row_ptr(nb + 1), col_idx(3 * nb), bi, bj, r, c, nnzb
    real(dp) :: vals(bs, bs, 3 * nb)
    nnzb = 0
    do bi = 1, nb
       row_ptr(bi) = nnzb + 1
       do bj = max(1, bi - 1), merge(bi, min(nb, bi + 1), lower)
          nnzb = nnzb + 1
          col_idx(nnzb) = bj
          do c = 1, bs
             do r = 1, bs
                vals(r, c, nnzb) = entry((bi - 1) * bs + r, (bj - 1) * bs + c, d0, dstep, eps)
             end do
          end do
       end do
    end do
    row_ptr(nb + 1) = nnzb + 1
    m = bsr_matrix(n, bs, row_ptr, col_idx(1:nnzb), vals(:, :, 1:nnzb), lower)
  end function banded

  !> y = M v from the full blocks of m (a matrix given in full, not as a lower triangle)
  function bsrmv(m, v) result(y)
    type(bsr_matrix), intent(in) :: m
    real(dp), intent(in) :: v(:)
    real(dp) :: y(size(v))
    integer :: bi, bj
    integer(8) :: p
    y = 0.0_dp
    do bi = 1, m%n / m%block_size
       do p = m%row_ptr(bi), m%row_ptr(bi + 1) - 1
          bj = m%col_idx(p)
          y((bi - 1) * bs + 1 : bi * bs) = y((bi - 1) * bs + 1 : bi * bs) + matmul(m%values(:, :, p), v((bj - 1) * bs + 1 : bj * bs))
       end do
    end do
  end function bsrmv

  subroutine check(name, ok)
    character(len=*), intent(in) :: name
    logical, intent(in) :: ok
    print "(a, 1x, a, 1x, l1)", "CHECK", name, ok
    if (.not. ok) nfail = nfail + 1
  end subroutine check

end program prog_bsr
