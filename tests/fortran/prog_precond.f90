!> The preconditioner slot as a Fortran user sees it: M through engine_set_sparse(eng, 3, ...) on a resident engine, and through the
!> keyword preconditioner= of the one-shot generic, as a csr_matrix and as a bsr_matrix.  A = the 5-point Laplacian of a 16 x 16 grid
!> plus a potential from an integer formula (the test rebuilds it in numpy), M = inv(L + mean(v) I) written as a full CSR / BSR matrix.
!> Every solve with M is checked against the plain "DPR" solve: same eigenvalues, fewer iterations.  Prints "CHECK name T|F" lines, the
!> eigenvalues and the iteration counts, and stops with a non-zero code on any F.
program prog_precond
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, csr_matrix, bsr_matrix
  use davidson_device
  use davidson_sparse, only: engine_set_sparse
  implicit none
  integer, parameter :: nx = 16, n = nx * nx, lowest = 4, bs = 4, nb = n / bs
  real(dp) :: dense(n, n), lap(n, n), minv(n, n), v(n)
  type(csr_matrix) :: a, mc
  type(bsr_matrix) :: mb
  type(davidson_engine) :: eng
  real(dp) :: ev_plain(lowest), ev_eng(lowest), ev_csr(lowest), ev_bsr(lowest)
  real(dp) :: x(n, lowest), x_eng(n, lowest), x_csr(n, lowest), x_bsr(n, lowest)
  integer :: it_plain, it_eng, it_csr, it_bsr, j, nfail

  nfail = 0
  call hamiltonian(lap, v)
  dense = lap
  do j = 1, n
     dense(j, j) = dense(j, j) + v(j)
  end do
  minv = lap
  do j = 1, n
     minv(j, j) = minv(j, j) + sum(v) / real(n, dp)
  end do
  call invert_spd(minv)
  a = as_csr(dense, .false.)
  mc = as_csr(minv, .true.)
  mb = as_bsr(minv)

  ! the resident engine: plain DPR first, then the same engine with M in slot 3
  call engine_create(eng, n, lowest, 10 * lowest, gev=.false.)
  call engine_set_sparse(eng, 1, a)
  call generalized_eigensolver(eng, ev_plain, x, lowest, "DPR", 400, 1d-8, it_plain, 10 * lowest)
  call engine_set_sparse(eng, 3, mc)
  call generalized_eigensolver(eng, ev_eng, x_eng, lowest, "DPR", 400, 1d-8, it_eng, 10 * lowest)
  call engine_destroy(eng)
  ! the one-shot call
  call generalized_eigensolver(a, ev_csr, x_csr, lowest, "DPR", 400, 1d-8, it_csr, preconditioner=mc)
  call generalized_eigensolver(a, ev_bsr, x_bsr, lowest, "DPR", 400, 1d-8, it_bsr, preconditioner=mb)

  call check("converged", max(it_plain, it_eng, it_csr, it_bsr) <= 400)
  call check("fewer_iterations_engine", it_eng < it_plain)
  call check("fewer_iterations_csr", it_csr < it_plain)
  call check("fewer_iterations_bsr", it_bsr < it_plain)
  call check("same_count_engine_and_one_shot", it_eng == it_csr)
  call check("eigenvalues_engine", maxval(abs(ev_eng - ev_plain)) < 1d-8)
  call check("eigenvalues_csr", maxval(abs(ev_csr - ev_plain)) < 1d-8)
  call check("eigenvalues_bsr", maxval(abs(ev_bsr - ev_plain)) < 1d-8)
  do j = 1, lowest
     call check("residual_engine", norm2(matmul(dense, x_eng(:, j)) - ev_eng(j) * x_eng(:, j)) < 1d-8)
     call check("residual_csr", norm2(matmul(dense, x_csr(:, j)) - ev_csr(j) * x_csr(:, j)) < 1d-8)
     call check("residual_bsr", norm2(matmul(dense, x_bsr(:, j)) - ev_bsr(j) * x_bsr(:, j)) < 1d-8)
  end do
  print "(a, 4i6)", "ITERS", it_plain, it_eng, it_csr, it_bsr
  print "(a, 4es26.17)", "EVALS_PLAIN", ev_plain
  print "(a, 4es26.17)", "EVALS_ENGINE", ev_eng
  print "(a, 4es26.17)", "EVALS_CSR", ev_csr
  print "(a, 4es26.17)", "EVALS_BSR", ev_bsr
  if (nfail > 0) error stop 1

contains

  subroutine hamiltonian(m, pot)
    real(dp), intent(out) :: m(n, n), pot(n)
    integer :: i, j, p
    m = 0.0_dp
    do i = 1, nx
       do j = 1, nx
          p = (i - 1) * nx + j
          m(p, p) = 4.0_dp
          pot(p) = 0.5_dp * real(mod(37 * p + 11, 101), dp) / 101.0_dp
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
  end subroutine hamiltonian

  !> in place, by Gauss-Jordan elimination without pivoting (the matrix is symmetric positive definite), then made exactly symmetric
  subroutine invert_spd(m)
    real(dp), intent(inout) :: m(n, n)
    real(dp) :: piv, col(n)
    integer :: k, j
    do k = 1, n
       piv = 1.0_dp / m(k, k)
       col = m(:, k)
       m(k, :) = m(k, :) * piv
       m(k, k) = piv
       do j = 1, n
          if (j == k) cycle
          m(j, :) = m(j, :) - col(j) * m(k, :)
          m(j, k) = -col(j) * piv
       end do
    end do
    m = 0.5_dp * (m + transpose(m))
  end subroutine invert_spd

  function as_csr(m, full) result(c)
    real(dp), intent(in) :: m(n, n)
    logical, intent(in) :: full                !< every entry is stored (a dense inverse), not only the non-zeros
    type(csr_matrix) :: c
    integer, allocatable :: row_ptr(:), col_idx(:)
    real(dp), allocatable :: vals(:)
    integer :: i, j, nnz
    allocate(row_ptr(n + 1), col_idx(n * n), vals(n * n))
    nnz = 0
    do i = 1, n
       row_ptr(i) = nnz + 1
       do j = 1, n
          if (full .or. m(i, j) /= 0.0_dp) then
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
    integer, allocatable :: row_ptr(:), col_idx(:)
    real(dp), allocatable :: vals(:, :, :)
    integer :: bi, bj, nnzb
    allocate(row_ptr(nb + 1), col_idx(nb * nb), vals(bs, bs, nb * nb))
    nnzb = 0
    do bi = 1, nb
       row_ptr(bi) = nnzb + 1
       do bj = 1, nb
          nnzb = nnzb + 1
          col_idx(nnzb) = bj
          vals(:, :, nnzb) = m((bi - 1) * bs + 1 : bi * bs, (bj - 1) * bs + 1 : bj * bs)
       end do
    end do
    row_ptr(nb + 1) = nnzb + 1
    c = bsr_matrix(n, bs, row_ptr, col_idx, vals, .false.)
  end function as_bsr

  subroutine check(name, ok)
    character(len=*), intent(in) :: name
    logical, intent(in) :: ok
    print "(a, 1x, a, 1x, l1)", "CHECK", name, ok
    if (.not. ok) nfail = nfail + 1
  end subroutine check

end program prog_precond
