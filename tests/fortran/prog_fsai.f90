!> The built preconditioner as a Fortran user sees it: engine_build_preconditioner(eng, sigma, level) on a resident engine whose
!> operator A is the 5-point Laplacian of a 20 x 20 grid plus a potential read from the file named on the command line (400 raw
!> float64 values: the test writes the potential of its case n400_std there).  Solves with "DPR" without M and with the built M of
!> level 1 and level 2; prints "CHECK name T|F" lines, the eigenvalues, the iteration counts and what engine_preconditioner_info
!> reports, and stops with a non-zero code on any F.
program prog_fsai
  use, intrinsic :: iso_c_binding, only: c_int64_t
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, csr_matrix
  use davidson_device
  use davidson_sparse, only: engine_set_sparse
  implicit none
  integer, parameter :: nx = 20, n = nx * nx, lowest = 4
  real(dp) :: dense(n, n), v(n)
  type(csr_matrix) :: a
  type(davidson_engine) :: eng
  real(dp) :: ev_plain(lowest), ev(lowest, 2), x(n, lowest)
  integer :: it_plain, it(2), j, level, nfail, unit, stat
  integer(c_int64_t) :: nnz(2), longest_row(2), longest_col(2)
  character(len=1024) :: path

  nfail = 0
  call get_command_argument(1, path)
  open(newunit=unit, file=trim(path), access="stream", form="unformatted", status="old", action="read")
  read(unit) v
  close(unit)
  call laplacian(dense)
  do j = 1, n
     dense(j, j) = dense(j, j) + v(j)
  end do
  a = as_csr(dense)

  call engine_create(eng, n, lowest, 10 * lowest, gev=.false.)
  call engine_set_sparse(eng, 1, a)
  call generalized_eigensolver(eng, ev_plain, x, lowest, "DPR", 400, 1d-8, it_plain, 10 * lowest)
  ! a refused build returns its status and leaves the engine usable
  call engine_build_preconditioner(eng, 0.0_dp, 4, stat)
  call check("level_4_is_refused", stat /= 0)
  do level = 1, 2
     call engine_build_preconditioner(eng, 0.0_dp, level)
     call engine_preconditioner_info(eng, nnz(level), longest_row(level), longest_col(level))
     call generalized_eigensolver(eng, ev(:, level), x, lowest, "DPR", 400, 1d-8, it(level), 10 * lowest)
     call check("eigenvalues", maxval(abs(ev(:, level) - ev_plain)) < 1d-8)
     do j = 1, lowest
        call check("residual", norm2(matmul(dense, x(:, j)) - ev(j, level) * x(:, j)) < 1d-8)
     end do
     call check("half_the_iterations", 2 * it(level) <= it_plain)
  end do
  call engine_destroy(eng)
  call check("converged", max(it_plain, it(1), it(2)) <= 400)
  print "(a, 3i6)", "ITERS", it_plain, it
  print "(a, 6i8)", "INFO", nnz(1), longest_row(1), longest_col(1), nnz(2), longest_row(2), longest_col(2)
  print "(a, 4es26.17)", "EVALS_PLAIN", ev_plain
  print "(a, 4es26.17)", "EVALS_LEVEL1", ev(:, 1)
  print "(a, 4es26.17)", "EVALS_LEVEL2", ev(:, 2)
  if (nfail > 0) error stop 1

contains

  subroutine laplacian(m)
    real(dp), intent(out) :: m(n, n)
    integer :: i, j, p
    m = 0.0_dp
    do i = 1, nx
       do j = 1, nx
          p = (i - 1) * nx + j
          m(p, p) = 4.0_dp
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
    integer, allocatable :: row_ptr(:), col_idx(:)
    real(dp), allocatable :: vals(:)
    integer :: i, j, nnz
    allocate(row_ptr(n + 1), col_idx(n * n), vals(n * n))
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

  subroutine check(name, ok)
    character(len=*), intent(in) :: name
    logical, intent(in) :: ok
    print "(a, 1x, a, 1x, l1)", "CHECK", name, ok
    if (.not. ok) nfail = nfail + 1
  end subroutine check

end program prog_fsai
