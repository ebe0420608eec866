!> Storage by diagonals as a Fortran user sees it: csr_matrix(..., diagonals=.true.) through the generic generalized_eigensolver, through
!> engine_set_sparse and - from device arrays (hipMalloc / hipMemcpy through bind(C) interfaces, as a hipfort user would) - through
!> engine_set_sparse_device(..., diagonals=.true.).  The matrix is the 5-point Laplacian of a 16 x 16 grid with a slightly perturbed
!> diagonal from an integer formula (the test rebuilds it in numpy).  A matrix with too many diagonals for its entries is refused through
!> stat and leaves the program running.  Prints "CHECK name T|F" lines and the eigenvalues, and stops with a non-zero code on any F.
program prog_dia
  use iso_c_binding
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, csr_matrix
  use davidson_device
  use davidson_sparse, only: engine_set_sparse, engine_set_sparse_device
  implicit none
  interface
     function hipMalloc(p, bytes) bind(C, name="hipMalloc") result(ierr)
       import :: c_ptr, c_size_t, c_int
       type(c_ptr) :: p
       integer(c_size_t), value :: bytes
       integer(c_int) :: ierr
     end function
     function hipMemcpy(dst, src, bytes, kind) bind(C, name="hipMemcpy") result(ierr)
       import :: c_ptr, c_size_t, c_int
       type(c_ptr), value :: dst, src
       integer(c_size_t), value :: bytes
       integer(c_int), value :: kind
       integer(c_int) :: ierr
     end function
     function hipFree(p) bind(C, name="hipFree") result(ierr)
       import :: c_ptr, c_int
       type(c_ptr), value :: p
       integer(c_int) :: ierr
     end function
  end interface
  integer, parameter :: nx = 16, n = nx * nx, lowest = 4
  integer(c_int), parameter :: host_to_device = 1
  real(dp) :: dense(n, n)
  type(csr_matrix), target :: a_csr, a_dia, a_low, a_wild
  type(davidson_engine) :: eng
  real(dp) :: ev_csr(lowest), ev_one(lowest), ev_eng(lowest), ev_dev(lowest), ev_pos(lowest), ev_low(lowest), ev_cheb(lowest)
  real(dp) :: x(n, lowest), x_one(n, lowest), x_eng(n, lowest), x_cheb(n, lowest)
  integer :: it_csr, it_one, it_eng, it_dev, it_pos, it_low, it_cheb, st, nfail
  type(c_ptr) :: d_rp, d_col, d_val

  nfail = 0
  call laplacian(dense)
  a_csr = as_csr(dense, .false., .false.)
  a_dia = as_csr(dense, .false., .true.)
  a_low = as_csr(dense, .true., .true.)
  call check("component", a_dia%diagonals .and. a_low%diagonals .and. a_low%lower .and. .not. a_csr%diagonals)

  ! the one call, without and with the flag
  call generalized_eigensolver(a_csr, ev_csr, x, lowest, "DPR", 400, 1d-8, it_csr)
  call generalized_eigensolver(a_dia, ev_one, x_one, lowest, "DPR", 400, 1d-8, it_one)
  call check("residual_one_call", residuals_small(x_one, ev_one) .and. it_one <= 400)
  call check("agrees_with_csr", maxval(abs(ev_one - ev_csr)) < 1d-9)

  ! an engine of the caller: from the csr_matrix, from device arrays, and the device entry called by position as before
  call engine_create(eng, n, lowest, 10 * lowest, gev=.false.)
  call engine_set_sparse(eng, 1, a_dia)
  call generalized_eigensolver(eng, ev_eng, x_eng, lowest, "DPR", 400, 1d-8, it_eng, 10 * lowest)
  call check("residual_engine", residuals_small(x_eng, ev_eng) .and. it_eng <= 400)

  call to_device(a_dia)
  call engine_set_sparse_device(eng, 1, n, d_rp, d_col, d_val, diagonals=.true.)
  call release()
  call generalized_eigensolver(eng, ev_dev, x, lowest, "DPR", 400, 1d-8, it_dev, 10 * lowest)
  call check("device_equals_host", all(transfer(ev_dev, 1_c_int64_t, lowest) == transfer(ev_eng, 1_c_int64_t, lowest)) &
       .and. it_dev == it_eng)

  call to_device(a_csr)
  call engine_set_sparse_device(eng, 1, n, d_rp, d_col, d_val, 1, .false., 64, 32, st)
  call release()
  call generalized_eigensolver(eng, ev_pos, x, lowest, "DPR", 400, 1d-8, it_pos, 10 * lowest)
  call check("positional_call", st == 0 .and. maxval(abs(ev_pos - ev_csr)) < 1d-9)

  call to_device(a_low)
  call engine_set_sparse_device(eng, 1, n, d_rp, d_col, d_val, lower=.true., stat=st, diagonals=.true.)
  call release()
  call generalized_eigensolver(eng, ev_low, x, lowest, "DPR", 400, 1d-8, it_low, 10 * lowest)
  call check("lower_equals_full", st == 0 .and. maxval(abs(ev_low - ev_eng)) < 1d-12 .and. it_low == it_eng)

  ! too many diagonals for its entries: refused, reported through stat, the engine takes the next matrix
  a_wild = wild()
  call to_device(a_wild)
  call engine_set_sparse_device(eng, 1, n, d_rp, d_col, d_val, stat=st, diagonals=.true.)
  call release()
  call check("refused_with_stat", st /= 0)
  call engine_set_sparse(eng, 1, a_dia)
  call generalized_eigensolver(eng, ev_cheb, x_cheb, lowest, "CHEB", 400, 1d-8, it_cheb, 10 * lowest)
  call check("residual_cheb", residuals_small(x_cheb, ev_cheb) .and. it_cheb < it_eng)
  call engine_destroy(eng)

  print "(a, 7i6)", "ITERS", it_csr, it_one, it_eng, it_dev, it_pos, it_low, it_cheb
  print "(a, 4es26.17)", "EVALS_ONE_CALL", ev_one
  print "(a, 4es26.17)", "EVALS_ENGINE", ev_eng
  print "(a, 4es26.17)", "EVALS_DEVICE", ev_dev
  print "(a, 4es26.17)", "EVALS_CHEB", ev_cheb
  if (nfail > 0) error stop 1

contains

  logical function residuals_small(vec, ev)
    real(dp), intent(in) :: vec(n, lowest), ev(lowest)
    integer :: j
    residuals_small = .true.
    do j = 1, lowest
       residuals_small = residuals_small .and. norm2(matmul(dense, vec(:, j)) - ev(j) * vec(:, j)) < 1d-8
    end do
  end function residuals_small

  subroutine to_device(m)
    type(csr_matrix), target, intent(in) :: m
    integer(c_size_t) :: brp, bcol, bval
    brp = 8_c_size_t * size(m%row_ptr, kind=c_size_t)
    bcol = 4_c_size_t * size(m%col_idx, kind=c_size_t)
    bval = 8_c_size_t * size(m%values, kind=c_size_t)
    if (hipMalloc(d_rp, brp) /= 0 .or. hipMalloc(d_col, bcol) /= 0 .or. hipMalloc(d_val, bval) /= 0) error stop "hipMalloc"
    if (hipMemcpy(d_rp, c_loc(m%row_ptr), brp, host_to_device) /= 0) error stop "hipMemcpy"
    if (hipMemcpy(d_col, c_loc(m%col_idx), bcol, host_to_device) /= 0) error stop "hipMemcpy"
    if (hipMemcpy(d_val, c_loc(m%values), bval, host_to_device) /= 0) error stop "hipMemcpy"
  end subroutine to_device

  subroutine release()
    if (hipFree(d_rp) /= 0 .or. hipFree(d_col) /= 0 .or. hipFree(d_val) /= 0) error stop "hipFree"
  end subroutine release

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

  function as_csr(m, lower, diagonals) result(c)
    real(dp), intent(in) :: m(n, n)
    logical, intent(in) :: lower, diagonals
    type(csr_matrix) :: c
    integer :: row_ptr(n + 1), col_idx(5 * n), i, j, nnz
    real(dp) :: vals(5 * n)
    nnz = 0
    do i = 1, n
       row_ptr(i) = nnz + 1
       do j = 1, merge(i, n, lower)
          if (m(i, j) /= 0.0_dp) then
             nnz = nnz + 1
             col_idx(nnz) = j
             vals(nnz) = m(i, j)
          end if
       end do
    end do
    row_ptr(n + 1) = nnz + 1
    c = csr_matrix(n, row_ptr, col_idx(1:nnz), vals(1:nnz), lower, diagonals=diagonals)
  end function as_csr

  !> the diagonal and one entry per row at a scattered column: some hundred different offsets for 2 n entries
  function wild() result(c)
    type(csr_matrix) :: c
    integer :: row_ptr(n + 1), col_idx(2 * n), i
    real(dp) :: vals(2 * n)
    do i = 1, n
       row_ptr(i) = 2 * i - 1
       col_idx(2 * i - 1) = i
       vals(2 * i - 1) = 4.0_dp
       col_idx(2 * i) = mod(37 * i * i + 11 * i, n) + 1
       vals(2 * i) = 0.01_dp
    end do
    row_ptr(n + 1) = 2 * n + 1
    c = csr_matrix(n, row_ptr, col_idx, vals)
  end function wild

  subroutine check(name, ok)
    character(len=*), intent(in) :: name
    logical, intent(in) :: ok
    print "(a, 1x, a, 1x, l1)", "CHECK", name, ok
    if (.not. ok) nfail = nfail + 1
  end subroutine check

end program prog_dia
