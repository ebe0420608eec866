!> The built block preconditioner as a Fortran user sees it: engine_build_block_preconditioner(eng, sigma, level) on a resident engine
!> whose operator A is a bsr_matrix, and on one whose operator A is a zcsr_matrix (engine_set_hermitian).  Both matrices travel in the
!> file named on the command line (stream of int32 / float64, written by tests/test_bfsai_fortran.py): nb, bs, nnzb, the 1-based block
!> row offsets and block columns, the blocks values(bs, bs, nnzb), sigma; then nc, nnz, the 1-based offsets and columns and the (re, im)
!> values of the complex matrix.  Solves with "DPR" without M and with the built M; prints "CHECK name T|F" lines, the eigenvalues, the
!> iteration counts and what engine_block_preconditioner_info reports, and stops with a non-zero code on any F.
program prog_bfsai
  use, intrinsic :: iso_c_binding, only: c_int, c_int64_t
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, bsr_matrix, zcsr_matrix
  use davidson_device
  use davidson_sparse, only: engine_set_sparse
  use davidson_hermitian, only: engine_set_hermitian
  implicit none
  integer, parameter :: lowest = 4
  type(bsr_matrix) :: a
  type(zcsr_matrix) :: h
  type(davidson_engine) :: eng
  real(dp) :: sigma
  real(dp), allocatable :: ev_plain(:), ev(:, :), x(:, :)
  integer :: it_plain, it(2), level, nfail, unit, stat, n, herm_plain, herm_it
  integer(c_int) :: bsize(3)
  integer(c_int64_t) :: nnzb(3), longest_row(3), longest_col(3)
  character(len=1024) :: path

  nfail = 0
  call get_command_argument(1, path)
  open(newunit=unit, file=trim(path), access="stream", form="unformatted", status="old", action="read")
  call read_bsr(unit, a, sigma)
  call read_zcsr(unit, h)
  close(unit)

  ! ---- a bsr_matrix
  n = a%n
  allocate(ev_plain(lowest), ev(lowest, 2), x(n, lowest))
  call engine_create(eng, n, lowest, 10 * lowest, gev=.false.)
  call engine_set_sparse(eng, 1, a)
  call generalized_eigensolver(eng, ev_plain, x, lowest, "DPR", 400, 1d-8, it_plain, 10 * lowest)
  ! a refused build returns its status and leaves the engine usable
  call engine_build_block_preconditioner(eng, sigma, 4, stat)
  call check("level_4_is_refused", stat /= 0)
  call engine_block_preconditioner_info(eng, bsize(3), nnzb(3), longest_row(3), longest_col(3))
  call check("nothing_is_built", bsize(3) == 0 .and. nnzb(3) == 0)
  do level = 1, 2
     call engine_build_block_preconditioner(eng, sigma, level)
     call engine_block_preconditioner_info(eng, bsize(level), nnzb(level), longest_row(level), longest_col(level))
     call generalized_eigensolver(eng, ev(:, level), x, lowest, "DPR", 400, 1d-8, it(level), 10 * lowest)
     call check("eigenvalues", maxval(abs(ev(:, level) - ev_plain)) < 1d-8)
     call check("fewer_iterations", it(level) < it_plain)
  end do
  call engine_destroy(eng)
  call check("converged", max(it_plain, it(1), it(2)) <= 400)
  print "(a, 3i6)", "ITERS_BSR", it_plain, it
  print "(a, 8i8)", "INFO_BSR", bsize(1), nnzb(1), longest_row(1), longest_col(1), bsize(2), nnzb(2), longest_row(2), longest_col(2)
  print "(a, 4es26.17)", "EVALS_PLAIN", ev_plain
  print "(a, 4es26.17)", "EVALS_LEVEL1", ev(:, 1)
  print "(a, 4es26.17)", "EVALS_LEVEL2", ev(:, 2)
  deallocate(ev_plain, ev, x)

  ! ---- a zcsr_matrix through its real form: block size 2, the default level
  n = 2 * h%n
  allocate(ev_plain(2 * lowest), ev(2 * lowest, 1), x(n, 2 * lowest))
  call engine_create(eng, n, 2 * lowest, 20 * lowest, gev=.false.)
  call engine_set_hermitian(eng, 1, h)
  call generalized_eigensolver(eng, ev_plain, x, 2 * lowest, "DPR", 400, 1d-8, herm_plain, 20 * lowest)
  call engine_build_block_preconditioner(eng, 0.0_dp)
  call engine_block_preconditioner_info(eng, bsize(3), nnzb(3), longest_row(3), longest_col(3))
  call generalized_eigensolver(eng, ev(:, 1), x, 2 * lowest, "DPR", 400, 1d-8, herm_it, 20 * lowest)
  call engine_destroy(eng)
  call check("hermitian_eigenvalues", maxval(abs(ev(:, 1) - ev_plain)) < 1d-8)
  call check("hermitian_fewer_iterations", herm_it < herm_plain)
  call check("hermitian_block_size", bsize(3) == 2)
  print "(a, 2i6)", "ITERS_HERM", herm_plain, herm_it
  print "(a, 4i8)", "INFO_HERM", bsize(3), nnzb(3), longest_row(3), longest_col(3)
  print "(a, 8es26.17)", "EVALS_HERM", ev(:, 1)
  if (nfail > 0) error stop 1

contains

  subroutine read_bsr(u, m, shift)
    integer, intent(in) :: u
    type(bsr_matrix), intent(out) :: m
    real(dp), intent(out) :: shift
    integer(c_int) :: head(3)
    integer(c_int), allocatable :: rp(:), col(:)
    real(dp), allocatable :: vals(:, :, :)
    read(u) head
    allocate(rp(head(1) + 1), col(head(3)), vals(head(2), head(2), head(3)))
    read(u) rp, col, vals, shift
    m = bsr_matrix(int(head(1) * head(2)), int(head(2)), int(rp), int(col), vals, .false.)
  end subroutine read_bsr

  subroutine read_zcsr(u, m)
    integer, intent(in) :: u
    type(zcsr_matrix), intent(out) :: m
    integer(c_int) :: head(2)
    integer(c_int), allocatable :: rp(:), col(:)
    real(dp), allocatable :: re_im(:, :)
    read(u) head
    allocate(rp(head(1) + 1), col(head(2)), re_im(2, head(2)))
    read(u) rp, col, re_im
    m = zcsr_matrix(int(head(1)), int(rp), int(col), cmplx(re_im(1, :), re_im(2, :), dp))
  end subroutine read_zcsr

  subroutine check(name, ok)
    character(len=*), intent(in) :: name
    logical, intent(in) :: ok
    print "(a, 1x, a, 1x, l1)", "CHECK", name, ok
    if (.not. ok) nfail = nfail + 1
  end subroutine check

end program prog_bfsai
