!> The block-diagonal preconditioned correction as a Fortran user sees it: method "BDPR" of the generic generalized_eigensolver on a
!> bsr_matrix.  A block-structured matrix of 4 x 4 blocks - strong coupling inside a block, weak hops to the neighbouring block row - and
!> an overlap matrix of the same structure around the identity, both from integer formulas (the test rebuilds them in numpy), solved as a
!> standard and as a generalized problem, and once with scalar "DPR" for the iteration count.  Prints "CHECK name T|F" lines, the
!> eigenvalues and the iteration counts, and stops with a non-zero code on any F.
program prog_bdpr
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, bsr_matrix
  implicit none
  integer, parameter :: n = 240, lowest = 4, bs = 4, nb = n / bs
  type(bsr_matrix) :: a, b
  real(dp) :: ev(lowest), ev_gen(lowest), ev_dpr(lowest)
  real(dp) :: x(n, lowest), x_gen(n, lowest), x_dpr(n, lowest)
  integer :: it, it_gen, it_dpr, j, nfail

  nfail = 0
  a = blocks(.false.)
  b = blocks(.true.)

  call generalized_eigensolver(a, ev, x, lowest, "BDPR", 300, 1d-8, it)
  call generalized_eigensolver(a, ev_gen, x_gen, lowest, "BDPR", 300, 1d-8, it_gen, 10 * lowest, b)
  call generalized_eigensolver(a, ev_dpr, x_dpr, lowest, "DPR", 300, 1d-8, it_dpr)

  do j = 1, lowest
     call check("residual_std", norm2(bsrmv(a, x(:, j)) - ev(j) * x(:, j)) < 1d-8)
     call check("residual_gen", norm2(bsrmv(a, x_gen(:, j)) - ev_gen(j) * bsrmv(b, x_gen(:, j))) < 1d-8)
  end do
  print "(a, 3i6)", "ITERS", it, it_gen, it_dpr
  print "(a, 4es26.17)", "EVALS_STD", ev
  print "(a, 4es26.17)", "EVALS_GEN", ev_gen
  if (nfail > 0) error stop 1

contains

  !> entry (r, c) of block (bi, bj), bj = bi - 1, bi or bi + 1, of A or (overlap) of B
  pure real(dp) function entry(bi, bj, r, c, overlap)
    integer, intent(in) :: bi, bj, r, c
    logical, intent(in) :: overlap
    if (bj == bi) then
       if (overlap) then
          entry = 0.1_dp * (real(mod(7 * bi + 2 * (r + c) + r * c, 13), dp) / 13.0_dp - 0.5_dp)
          if (r == c) entry = entry + 1.0_dp
       else
          entry = real(mod(17 * bi + 5 * (r + c) + 3 * r * c, 11), dp) / 11.0_dp - 0.5_dp
          if (r == c) entry = entry + (real(r - 1, dp) * 1.0_dp + 0.01_dp * real(bi - 1, dp))
       end if
    else if (bj == bi - 1) then
       if (overlap) then
          entry = 0.01_dp * (real(mod(3 * bi + 5 * r + 2 * c, 19), dp) / 19.0_dp - 0.5_dp)
       else
          entry = 0.05_dp * (real(mod(5 * bi + 3 * r + 7 * c, 17), dp) / 17.0_dp - 0.5_dp)
       end if
    else
       entry = entry_above(bi, bj, r, c, overlap)        ! the transpose of block (bj, bi)
    end if
  end function entry

  pure real(dp) function entry_above(bi, bj, r, c, overlap)
    integer, intent(in) :: bi, bj, r, c
    logical, intent(in) :: overlap
    if (overlap) then
       entry_above = 0.01_dp * (real(mod(3 * bj + 5 * c + 2 * r, 19), dp) / 19.0_dp - 0.5_dp)
    else
       entry_above = 0.05_dp * (real(mod(5 * bj + 3 * c + 7 * r, 17), dp) / 17.0_dp - 0.5_dp)
    end if
  end function entry_above

  function blocks(overlap) result(m)
    logical, intent(in) :: overlap
    type(bsr_matrix) :: m
    integer :: row_ptr(nb + 1), col_idx(3 * nb), bi, bj, r, c, nnzb
    real(dp) :: vals(bs, bs, 3 * nb)
    nnzb = 0
    do bi = 1, nb
       row_ptr(bi) = nnzb + 1
       do bj = max(1, bi - 1), min(nb, bi + 1)
          nnzb = nnzb + 1
          col_idx(nnzb) = bj
          do c = 1, bs
             do r = 1, bs
                vals(r, c, nnzb) = entry(bi, bj, r, c, overlap)
             end do
          end do
       end do
    end do
    row_ptr(nb + 1) = nnzb + 1
    m = bsr_matrix(n, bs, row_ptr, col_idx(1:nnzb), vals(:, :, 1:nnzb), .false.)
  end function blocks

  !> y = M v from the full blocks of m
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

end program prog_bdpr
