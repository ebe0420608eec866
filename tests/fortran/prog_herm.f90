!> Complex Hermitian operators as a Fortran user sees them.
!> Without an argument (GPU): a zcsr_matrix through the one-shot generic - a standard problem and a pencil - through
!> engine_set_hermitian on a resident engine of the real order 2 n with hermitian_eigenpairs, and engine_update_hermitian_values against
!> a fresh solve of the new values.  The matrix: a 12 x 12 square lattice with Peierls phases (site p = (ix - 1) nx + iy: on-site
!> 4 + 0.3 mod(37 p + 11, 101) / 101 + 0.05 ((ix - 6.5)^2 + (iy - 6.5)^2), hopping -1 along y and -exp(2 pi i iy / 8) along x), given by
!> its lower triangle; the pencil's S has 1 on the diagonal and 0.05 i along y.  Prints "EVALS_<name>" and "ITERS".
!> "solve <file>" (GPU): the matrix of the file - "n lowest has_s method", then for A and (has_s = 1) for S "nnz", row_ptr, col_idx
!> (1-based) and the (re, im) values - through engine_set_hermitian on a resident engine, whose real-form pairs are printed ("THETA",
!> "V") with the complex pairs hermitian_eigenpairs takes from them ("LAMBDA", "X"), and through the zcsr_matrix specific of the generic
!> ("LAMBDA1", "X1"); "ITERS" holds both counts.
!> "<file>" alone (CPU, no engine call): hermitian_eigenpairs on the real-form pairs of the file - "n lowest has_s", theta, v by
!> columns, and with has_s = 1 "nnz", row_ptr, col_idx and the (re, im) values of S - printed as "LAMBDA" and "X" lines.
program prog_herm
  use, intrinsic :: iso_c_binding
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, zcsr_matrix
  use davidson_device
  use davidson_sparse, only: engine_keep_value_map
  use davidson_hermitian, only: engine_set_hermitian, engine_update_hermitian_values, hermitian_eigenpairs
  implicit none
  integer, parameter :: nx = 12, n = nx * nx, lowest = 4
  character(len=1024) :: path
  type(zcsr_matrix) :: a, a2, s
  type(davidson_engine) :: eng
  real(dp) :: ev(lowest, 5), theta(2 * lowest), v(2 * n, 2 * lowest)
  complex(dp) :: x(n, lowest), xs(n, lowest)
  integer :: it(5)

  if (command_argument_count() >= 2) then
     call get_command_argument(2, path)
     call solve_from_file(trim(path))
     stop
  end if
  if (command_argument_count() >= 1) then
     call get_command_argument(1, path)
     call extract_from_file(trim(path))
     stop
  end if

  call lattice(a, s)
  a2 = a
  a2%values = 1.5_dp * a%values

  ! 1: the one-shot generic; 2: the pencil
  call generalized_eigensolver(a, ev(:, 1), x, lowest, "DPR", 400, 1d-8, it(1))
  call generalized_eigensolver(a, ev(:, 2), xs, lowest, "GJD", 400, 1d-8, it(2), second_matrix=s)
  ! 3: a resident engine of the real order 2 n; 4: after new values in the order of the set call; 5: a fresh solve of those values
  call engine_create(eng, 2 * n, 2 * lowest, 20 * lowest, gev=.false.)
  call engine_keep_value_map(eng, 1, .true.)
  call engine_set_hermitian(eng, 1, a)
  call generalized_eigensolver(eng, theta, v, 2 * lowest, "DPR", 400, 1d-8, it(3), 20 * lowest)
  call hermitian_eigenpairs(theta, v, lowest, ev(:, 3), x)
  call engine_update_hermitian_values(eng, 1, a2%values)
  call generalized_eigensolver(eng, theta, v, 2 * lowest, "DPR", 400, 1d-8, it(4), 20 * lowest)
  call hermitian_eigenpairs(theta, v, lowest, ev(:, 4), x)
  call engine_destroy(eng)
  call generalized_eigensolver(a2, ev(:, 5), x, lowest, "DPR", 400, 1d-8, it(5))

  print "(a, 4es25.16)", "EVALS_ONESHOT", ev(:, 1)
  print "(a, 4es25.16)", "EVALS_PENCIL", ev(:, 2)
  print "(a, 4es25.16)", "EVALS_ENGINE", ev(:, 3)
  print "(a, 4es25.16)", "EVALS_UPDATED", ev(:, 4)
  print "(a, 4es25.16)", "EVALS_SCALED", ev(:, 5)
  print "(a, 5i6)", "ITERS", it
  if (maxval(it) >= 400) error stop 1

contains

  !> the lattice and the overlap by their lower triangles, the columns of a row ascending
  subroutine lattice(h, ov)
    type(zcsr_matrix), intent(out) :: h, ov
    integer :: rp(n + 1), col(3 * n), scol(2 * n), srp(n + 1), ix, iy, p, cnt, scnt
    complex(dp) :: val(3 * n), sval(2 * n)
    real(dp), parameter :: pi = 3.14159265358979323846_dp
    cnt = 0
    scnt = 0
    do ix = 1, nx
       do iy = 1, nx
          p = (ix - 1) * nx + iy
          rp(p) = cnt + 1
          srp(p) = scnt + 1
          if (ix > 1) then          ! entry (p, p - nx): the hop along x from the site with the same iy
             cnt = cnt + 1; col(cnt) = p - nx
             val(cnt) = -exp(cmplx(0.0_dp, 2.0_dp * pi * real(iy, dp) / 8.0_dp, dp))
          end if
          if (iy > 1) then
             cnt = cnt + 1; col(cnt) = p - 1; val(cnt) = (-1.0_dp, 0.0_dp)
             scnt = scnt + 1; scol(scnt) = p - 1; sval(scnt) = (0.0_dp, 0.05_dp)
          end if
          cnt = cnt + 1; col(cnt) = p
          val(cnt) = cmplx(4.0_dp + 0.3_dp * real(mod(37 * p + 11, 101), dp) / 101.0_dp &
               + 0.05_dp * ((real(ix, dp) - 6.5_dp) ** 2 + (real(iy, dp) - 6.5_dp) ** 2), 0.0_dp, dp)
          scnt = scnt + 1; scol(scnt) = p; sval(scnt) = (1.0_dp, 0.0_dp)
       end do
    end do
    rp(n + 1) = cnt + 1
    srp(n + 1) = scnt + 1
    h = zcsr_matrix(n, rp, col(1:cnt), val(1:cnt), lower=.true.)
    ov = zcsr_matrix(n, srp, scol(1:scnt), sval(1:scnt), lower=.true.)
  end subroutine lattice

  subroutine read_zcsr(u, nn, a)
    integer, intent(in) :: u, nn
    type(zcsr_matrix), intent(out) :: a
    integer :: nnz
    integer, allocatable :: rp(:), col(:)
    real(dp), allocatable :: re_im(:, :)
    read(u, *) nnz
    allocate(rp(nn + 1), col(nnz), re_im(2, nnz))
    read(u, *) rp
    read(u, *) col
    read(u, *) re_im
    a = zcsr_matrix(nn, rp, col, cmplx(re_im(1, :), re_im(2, :), dp))
  end subroutine read_zcsr

  subroutine print_complex(name, xx)
    character(len=*), intent(in) :: name
    complex(dp), intent(in) :: xx(:, :)
    integer :: i, j
    do j = 1, size(xx, 2)
       do i = 1, size(xx, 1)
          print "(a, 2es25.16)", name, real(xx(i, j), dp), aimag(xx(i, j))
       end do
    end do
  end subroutine print_complex

  subroutine solve_from_file(file)
    character(len=*), intent(in) :: file
    character(len=16) :: method
    integer :: nn, ll, has_s, u, its(2), i, j
    type(zcsr_matrix) :: ma, ms
    type(davidson_engine) :: en
    real(dp), allocatable :: th(:), vv(:, :), lam(:), lam1(:)
    complex(dp), allocatable :: xx(:, :), xx1(:, :)
    open(newunit=u, file=file, status="old", action="read")
    read(u, *) nn, ll, has_s, method
    call read_zcsr(u, nn, ma)
    if (has_s /= 0) call read_zcsr(u, nn, ms)
    close(u)
    allocate(th(2 * ll), vv(2 * nn, 2 * ll), lam(ll), lam1(ll), xx(nn, ll), xx1(nn, ll))
    call engine_create(en, 2 * nn, 2 * ll, 20 * ll, gev=has_s /= 0)
    call engine_set_hermitian(en, 1, ma)
    if (has_s /= 0) call engine_set_hermitian(en, 2, ms)
    call generalized_eigensolver(en, th, vv, 2 * ll, trim(method), 400, 1d-8, its(1), 20 * ll)
    call engine_destroy(en)
    if (has_s /= 0) then
       call hermitian_eigenpairs(th, vv, ll, lam, xx, ms)
       call generalized_eigensolver(ma, lam1, xx1, ll, trim(method), 400, 1d-8, its(2), second_matrix=ms)
    else
       call hermitian_eigenpairs(th, vv, ll, lam, xx)
       call generalized_eigensolver(ma, lam1, xx1, ll, trim(method), 400, 1d-8, its(2))
    end if
    print "(a, 2i6)", "ITERS", its
    print "(a, *(es25.16))", "THETA", th
    do j = 1, 2 * ll
       do i = 1, 2 * nn
          print "(a, es25.16)", "V", vv(i, j)
       end do
    end do
    print "(a, *(es25.16))", "LAMBDA ", lam
    call print_complex("X ", xx)
    print "(a, *(es25.16))", "LAMBDA1", lam1
    call print_complex("X1", xx1)
  end subroutine solve_from_file

  subroutine extract_from_file(file)
    character(len=*), intent(in) :: file
    integer :: nn, ll, has_s, nnz, u, j, i
    real(dp), allocatable :: th(:), vv(:, :), lam(:), re_im(:, :)
    complex(dp), allocatable :: xx(:, :)
    integer, allocatable :: rp(:), col(:)
    type(zcsr_matrix) :: ov
    open(newunit=u, file=file, status="old", action="read")
    read(u, *) nn, ll, has_s
    allocate(th(2 * ll), vv(2 * nn, 2 * ll), lam(ll), xx(nn, ll))
    read(u, *) th
    read(u, *) vv
    if (has_s /= 0) then
       read(u, *) nnz
       allocate(rp(nn + 1), col(nnz), re_im(2, nnz))
       read(u, *) rp
       read(u, *) col
       read(u, *) re_im
       ov = zcsr_matrix(nn, rp, col, cmplx(re_im(1, :), re_im(2, :), dp))
       call hermitian_eigenpairs(th, vv, ll, lam, xx, ov)
    else
       call hermitian_eigenpairs(th, vv, ll, lam, xx)
    end if
    close(u)
    print "(a, *(es25.16))", "LAMBDA", lam
    do j = 1, ll
       do i = 1, nn
          print "(a, 2es25.16)", "X", real(xx(i, j), dp), aimag(xx(i, j))
       end do
    end do
  end subroutine extract_from_file
end program prog_herm
