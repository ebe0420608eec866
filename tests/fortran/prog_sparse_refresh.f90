!> New values on a kept pattern from Fortran, the loop of an SCF iteration: a banded csr_matrix is set once with
!> engine_keep_value_map on and solved; engine_update_sparse_values then moves the values of a second matrix of the same pattern into
!> the operator and the engine solves again.  The second solve must be bit-identical to the solve of a fresh engine_set_sparse of the
!> second matrix; the same pattern as a bsr_matrix with blocks of one takes the rank-3 specific.  Prints "CHECK name T|F" lines and both
!> spectra, and stops with a non-zero code on any F.
program prog_sparse_refresh
  use iso_c_binding
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, csr_matrix, bsr_matrix
  use davidson_device
  use davidson_sparse, only: engine_set_sparse, engine_keep_value_map, engine_update_sparse_values
  implicit none
  integer, parameter :: n = 1200, lowest = 4
  type(csr_matrix) :: a1, a2
  type(bsr_matrix) :: b1
  type(davidson_engine) :: eng, fresh
  real(dp) :: ev_first(lowest), ev_second(lowest), ev_fresh(lowest), ev_bsr(lowest), x(n, lowest)
  real(dp), allocatable :: blocks(:, :, :)
  integer :: it_first, it_second, it_fresh, it_bsr, nfail

  nfail = 0
  a1 = banded(1.0_dp, 1.0_dp, 0.3_dp)
  a2 = banded(2.0_dp, 1.5_dp, 0.2_dp)

  call engine_create(eng, n, lowest, 10 * lowest, gev=.false.)
  call engine_keep_value_map(eng, 1, .true.)
  call engine_set_sparse(eng, 1, a1)
  call generalized_eigensolver(eng, ev_first, x, lowest, "DPR", 1000, 1d-8, it_first, 10 * lowest)
  call engine_update_sparse_values(eng, 1, a2%values)
  call generalized_eigensolver(eng, ev_second, x, lowest, "DPR", 1000, 1d-8, it_second, 10 * lowest)

  call engine_create(fresh, n, lowest, 10 * lowest, gev=.false.)
  call engine_set_sparse(fresh, 1, a2)
  call generalized_eigensolver(fresh, ev_fresh, x, lowest, "DPR", 1000, 1d-8, it_fresh, 10 * lowest)
  call engine_destroy(fresh)
  call check("update_equals_fresh_set", all(transfer(ev_second, 1_c_int64_t, lowest) == transfer(ev_fresh, 1_c_int64_t, lowest)) &
       .and. it_second == it_fresh)
  call check("values_changed", minval(abs(ev_second - ev_first)) > 0.5_dp)

  ! the same pattern in blocks of one: values(1, 1, nnz)
  b1 = bsr_matrix(n, 1, int(a1%row_ptr), int(a1%col_idx), reshape(a1%values, [1, 1, size(a1%values)]), .true.)
  call engine_set_sparse(eng, 1, b1)
  blocks = reshape(a2%values, [1, 1, size(a2%values)])
  call engine_update_sparse_values(eng, 1, blocks)
  call generalized_eigensolver(eng, ev_bsr, x, lowest, "DPR", 1000, 1d-8, it_bsr, 10 * lowest)
  call check("bsr_update", maxval(abs(ev_bsr - ev_fresh)) < 1d-8)
  call engine_destroy(eng)

  print "(a, 4i6)", "ITERS", it_first, it_second, it_fresh, it_bsr
  print "(a, 4es26.17)", "EVALS_FIRST", ev_first
  print "(a, 4es26.17)", "EVALS_SECOND", ev_second
  if (nfail > 0) error stop 1

contains

  !> the lower triangle of: d0 + dstep * (i - 1) on the diagonal, eps on the first and eps / 2 on the second off-diagonals
  function banded(d0, dstep, eps) result(m)
    real(dp), intent(in) :: d0, dstep, eps
    type(csr_matrix) :: m
    integer :: row_ptr(n + 1), col_idx(3 * n), i, j, nnz
    real(dp) :: vals(3 * n)
    nnz = 0
    do i = 1, n
       row_ptr(i) = nnz + 1
       do j = max(1, i - 2), i
          nnz = nnz + 1
          col_idx(nnz) = j
          select case (i - j)
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
    m = csr_matrix(n, row_ptr, col_idx(1:nnz), vals(1:nnz), .true.)
  end function banded

  subroutine check(name, ok)
    character(len=*), intent(in) :: name
    logical, intent(in) :: ok
    print "(a, 1x, a, 1x, l1)", "CHECK", name, ok
    if (.not. ok) nfail = nfail + 1
  end subroutine check

end program prog_sparse_refresh
