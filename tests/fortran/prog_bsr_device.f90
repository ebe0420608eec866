!> Device block arrays from Fortran: the banded bsr_matrix of prog_bsr (4 x 4 blocks) is copied to device memory with hipMalloc /
!> hipMemcpy (bind(C) interfaces, as a hipfort user would), handed to engine_set_block_sparse_device and solved through the engine
!> specific of generalized_eigensolver.  The eigenvalues must be bit-identical to the solve of the same bsr_matrix from host memory, for
!> the full matrix and for its lower block triangle.  A matrix refused with stat leaves the program running.  Prints "CHECK name T|F"
!> lines and the eigenvalues, and stops with a non-zero code on any F.
program prog_bsr_device
  use iso_c_binding
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, bsr_matrix
  use davidson_device
  use davidson_sparse, only: engine_set_sparse, engine_set_block_sparse_device
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
  integer, parameter :: n = 1200, lowest = 4, bs = 4, nb = n / bs
  integer(c_int), parameter :: host_to_device = 1
  type(bsr_matrix), target :: a, a_low
  type(davidson_engine) :: eng
  real(dp) :: ev_host(lowest), ev_dev(lowest), ev_low_host(lowest), ev_low(lowest), x(n, lowest)
  integer :: it_host, it_dev, it_low_host, it_low, st, nfail
  type(c_ptr) :: d_rp, d_col, d_val

  nfail = 0
  a = banded(1.0_dp, 1.0_dp, 0.3_dp, .false.)
  a_low = banded(1.0_dp, 1.0_dp, 0.3_dp, .true.)

  call engine_create(eng, n, lowest, 10 * lowest, gev=.false.)
  call engine_set_sparse(eng, 1, a)
  call generalized_eigensolver(eng, ev_host, x, lowest, "DPR", 1000, 1d-8, it_host, 10 * lowest)
  call engine_set_sparse(eng, 1, a_low)
  call generalized_eigensolver(eng, ev_low_host, x, lowest, "DPR", 1000, 1d-8, it_low_host, 10 * lowest)

  call to_device(a)
  call engine_set_block_sparse_device(eng, 1, n, bs, d_rp, d_col, d_val)
  call release()
  call generalized_eigensolver(eng, ev_dev, x, lowest, "DPR", 1000, 1d-8, it_dev, 10 * lowest)
  call check("device_equals_host", all(transfer(ev_dev, 1_c_int64_t, lowest) == transfer(ev_host, 1_c_int64_t, lowest)) &
       .and. it_dev == it_host)

  ! the full matrix declared lower: refused, reported through stat, the engine takes the next matrix
  call to_device(a)
  call engine_set_block_sparse_device(eng, 1, n, bs, d_rp, d_col, d_val, lower=.true., stat=st)
  call release()
  call check("refused_with_stat", st /= 0)
  call to_device(a_low)
  call engine_set_block_sparse_device(eng, 1, n, bs, d_rp, d_col, d_val, base=1, lower=.true., row_major=.false., row_ptr_bits=64, &
       col_bits=32, stat=st)
  call release()
  call check("lower_accepted", st == 0)
  call generalized_eigensolver(eng, ev_low, x, lowest, "DPR", 1000, 1d-8, it_low, 10 * lowest)
  call check("lower_device_equals_lower_host", all(transfer(ev_low, 1_c_int64_t, lowest) == transfer(ev_low_host, 1_c_int64_t, lowest)) &
       .and. it_low == it_low_host)
  call check("lower_equals_full", maxval(abs(ev_low - ev_host)) < 1d-12 .and. it_low == it_host)
  call engine_destroy(eng)

  print "(a, 4i6)", "ITERS", it_host, it_dev, it_low_host, it_low
  print "(a, 4es26.17)", "EVALS_HOST", ev_host
  print "(a, 4es26.17)", "EVALS_DEV", ev_dev
  if (nfail > 0) error stop 1

contains

  subroutine to_device(m)
    type(bsr_matrix), target, intent(in) :: m
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

  subroutine check(name, ok)
    character(len=*), intent(in) :: name
    logical, intent(in) :: ok
    print "(a, 1x, a, 1x, l1)", "CHECK", name, ok
    if (.not. ok) nfail = nfail + 1
  end subroutine check

end program prog_bsr_device
