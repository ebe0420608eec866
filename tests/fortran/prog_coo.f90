!> COO triples as a Fortran user sees them: a coo_matrix through the one-shot generic, through engine_set_sparse on a resident engine,
!> and engine_update_sparse_values with the values in the order of the triples.  The matrix: diagonal i + 1/2, couplings on the
!> offsets 1, 7 and 40 from an integer formula, every 5th coupling split into two terms at one position; the triples are emitted in a
!> scrambled order (p -> 1 + mod(p * 7919, nnz), a bijection as 7919 is prime and does not divide nnz).  The ROW FORM - a stable counting sort of
!> the triples by row, done here - goes through csr_matrix: the two must print the same digits.  Prints "EVALS_<name>" and "ITERS" lines.
program prog_coo
  use, intrinsic :: iso_c_binding
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, csr_matrix, coo_matrix
  use davidson_device
  use davidson_sparse, only: engine_set_sparse, engine_keep_value_map, engine_update_sparse_values
  implicit none
  integer, parameter :: n = 1200, lowest = 4
  integer, allocatable :: ri(:), ci(:), rs(:), cs(:), rp(:), csr_col(:), next(:)
  real(dp), allocatable :: vv(:), vs(:), csr_val(:)
  type(coo_matrix) :: a_coo
  type(csr_matrix) :: a_csr, a_csr2
  type(davidson_engine) :: eng
  real(dp) :: ev(lowest, 5), x(n, lowest)
  integer :: it(5), nnz, p, q, i, k

  call emit(ri, ci, vv)
  nnz = size(vv)
  if (mod(nnz, 7919) == 0) error stop "prog_coo: the scramble needs nnz not a multiple of 7919"
  allocate(rs(nnz), cs(nnz), vs(nnz))
  do p = 1, nnz
     q = 1 + int(mod(int(p, c_int64_t) * 7919_c_int64_t, int(nnz, c_int64_t)))
     rs(q) = ri(p); cs(q) = ci(p); vs(q) = vv(p)
  end do
  ! the row form of the scrambled triples
  allocate(rp(n + 1), next(n), csr_col(nnz), csr_val(nnz))
  rp = 0
  do p = 1, nnz
     rp(rs(p) + 1) = rp(rs(p) + 1) + 1
  end do
  rp(1) = 1
  do i = 1, n
     rp(i + 1) = rp(i + 1) + rp(i)
  end do
  next = rp(1:n)
  do p = 1, nnz
     k = next(rs(p)); next(rs(p)) = k + 1
     csr_col(k) = cs(p); csr_val(k) = vs(p)
  end do
  a_coo = coo_matrix(n, rs, cs, vs)
  a_csr = csr_matrix(n, rp, csr_col, csr_val)
  a_csr2 = csr_matrix(n, rp, csr_col, 1.5_dp * csr_val)

  ! 1: the row form as a csr_matrix; 2: the triples through the generic
  call generalized_eigensolver(a_csr, ev(:, 1), x, lowest, "DPR", 400, 1d-8, it(1))
  call generalized_eigensolver(a_coo, ev(:, 2), x, lowest, "DPR", 400, 1d-8, it(2))
  ! 3: a resident engine; 4: the same engine after new values in the order of the triples; 5: the csr_matrix with those values
  call engine_create(eng, n, lowest, 10 * lowest, gev=.false.)
  call engine_keep_value_map(eng, 1, .true.)
  call engine_set_sparse(eng, 1, a_coo)
  call generalized_eigensolver(eng, ev(:, 3), x, lowest, "DPR", 400, 1d-8, it(3), 10 * lowest)
  call engine_update_sparse_values(eng, 1, 1.5_dp * vs)
  call generalized_eigensolver(eng, ev(:, 4), x, lowest, "DPR", 400, 1d-8, it(4), 10 * lowest)
  call engine_destroy(eng)
  call generalized_eigensolver(a_csr2, ev(:, 5), x, lowest, "DPR", 400, 1d-8, it(5))

  print "(a, 4es25.16)", "EVALS_CSR", ev(:, 1)
  print "(a, 4es25.16)", "EVALS_COO", ev(:, 2)
  print "(a, 4es25.16)", "EVALS_ENGINE", ev(:, 3)
  print "(a, 4es25.16)", "EVALS_UPDATED", ev(:, 4)
  print "(a, 4es25.16)", "EVALS_CSR_SCALED", ev(:, 5)
  print "(a, 5i6)", "ITERS", it
  if (maxval(it) >= 400) error stop 1

contains

  !> the triples in assembly order: per row the diagonal, then the couplings of both triangles; every 5th coupling as two terms
  subroutine emit(r, c, v)
    integer, allocatable, intent(out) :: r(:), c(:)
    real(dp), allocatable, intent(out) :: v(:)
    integer, parameter :: offs(3) = [1, 7, 40]
    integer :: i, j, d, cnt, pass
    real(dp) :: w
    do pass = 1, 2
       cnt = 0
       do i = 1, n
          call put(i, i, real(i, dp) + 0.5_dp)
          do d = 1, 3
             do j = i - offs(d), i + offs(d), 2 * offs(d)
                if (j < 1 .or. j > n) cycle
                w = 0.01_dp * real(mod(13 * min(i, j) + 5 * offs(d), 17) + 1, dp) / 17.0_dp
                if (mod(min(i, j) + offs(d), 5) == 0) then
                   call put(i, j, 0.75_dp * w)
                   call put(i, j, 0.25_dp * w)
                else
                   call put(i, j, w)
                end if
             end do
          end do
       end do
       if (pass == 1) allocate(r(cnt), c(cnt), v(cnt))
    end do
  contains
    subroutine put(i, j, w)
      integer, intent(in) :: i, j
      real(dp), intent(in) :: w
      cnt = cnt + 1
      if (pass == 2) then
         r(cnt) = i; c(cnt) = j; v(cnt) = w
      end if
    end subroutine put
  end subroutine emit
end program prog_coo
