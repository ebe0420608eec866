!> Complex Hermitian CSR operators through their real form (include/davidson_hip_herm.h; DESIGN section 28).  A Hermitian matrix H of
!> order n has a real symmetric form of order 2 n: real and imaginary parts interleaved, v(2 i - 1) = Re x_i, v(2 i) = Im x_i, and every
!> entry a + i b the block [[a, -b], [b, a]] - a BSR operator with block size 2 on the pattern of H.  The engine is created with the real
!> order 2 n; engine_set_hermitian hands it a zcsr_matrix whose complex values are read where they lie.  Every eigenvalue of H appears
!> twice in the real form: a solve for `lowest` complex pairs is a solve for 2 * lowest real pairs, and hermitian_eigenpairs takes the
!> complex pairs out of the real invariant subspace.  The specific of generalized_eigensolver for a zcsr_matrix (module davidson) does
!> the three steps in one call.
module davidson_hermitian
  use, intrinsic :: iso_c_binding
  use numeric_kinds, only: dp
  use davidson_hip_c
  use davidson_engine_setup, only: davidson_engine
  implicit none
  private
  public :: zcsr_matrix, engine_set_hermitian, engine_set_hermitian_device, engine_update_hermitian_values, hermitian_eigenpairs

  !> A complex Hermitian matrix of order n in CSR form, 1-based: the entries of row i are col_idx / values(row_ptr(i) : row_ptr(i+1) - 1).
  !> lower = .true.: only the entries with column <= row are given (the engine mirrors the strict lower part as conjugates); .false.:
  !> every nonzero is given, and h_ji = conj(h_ij) is the caller's promise.  The diagonal entries are real (imaginary part +-0).
  type :: zcsr_matrix
     integer :: n = 0
     integer(c_int64_t), allocatable :: row_ptr(:)
     integer(c_int32_t), allocatable :: col_idx(:)
     complex(dp), allocatable :: values(:)
     logical :: lower = .false.
  end type zcsr_matrix

  !> zcsr_matrix(n, row_ptr, col_idx, values [, lower]) from default-kind integer arrays, 1-based
  interface zcsr_matrix
     module procedure new_zcsr_matrix
  end interface zcsr_matrix

  interface
     subroutine zheev(jobz, uplo, n, a, lda, w, work, lwork, rwork, info)
       import :: dp
       character, intent(in) :: jobz, uplo
       integer, intent(in) :: n, lda, lwork
       complex(dp), intent(inout) :: a(lda, *)
       real(dp), intent(out) :: w(*), rwork(*)
       complex(dp), intent(out) :: work(*)
       integer, intent(out) :: info
     end subroutine zheev
  end interface

contains

  function new_zcsr_matrix(n, row_ptr, col_idx, values, lower) result(a)
    integer, intent(in) :: n
    integer, intent(in) :: row_ptr(:), col_idx(:)
    complex(dp), intent(in) :: values(:)
    logical, intent(in), optional :: lower
    type(zcsr_matrix) :: a
    if (size(row_ptr) /= n + 1) then
       print *, "zcsr_matrix: row_ptr must hold n + 1 = ", n + 1, " offsets, not ", size(row_ptr)
       error stop
    end if
    if (size(col_idx) < row_ptr(n + 1) - 1 .or. size(values) < row_ptr(n + 1) - 1) then
       print *, "zcsr_matrix: row_ptr(n + 1) - 1 = ", row_ptr(n + 1) - 1, " entries, but col_idx / values hold ", size(col_idx), &
            " / ", size(values)
       error stop
    end if
    a%n = n
    a%row_ptr = int(row_ptr, c_int64_t)
    a%col_idx = int(col_idx, c_int32_t)
    a%values = values
    if (present(lower)) a%lower = lower
  end function new_zcsr_matrix

  !> Operator A (which = 1), B (which = 2) or the preconditioner M (which = 3) of an engine of order 2 * a%n from a zcsr_matrix: the
  !> engine keeps the 2 x 2 blocks of its slab in HBM, bit for bit those of the bsr_matrix of the expanded blocks, and applies them with
  !> its matrix-core BSR kernel.  The matrix is not referenced after the call.
  subroutine engine_set_hermitian(eng, which, a)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    type(zcsr_matrix), intent(in), target :: a
    real(dp), pointer :: pairs(:)
    real(dp) :: nothing(2)
    integer(c_int) :: tri
    tri = merge(DAV_CSR_LOWER, DAV_CSR_FULL, a%lower)
    if (2 * a%n /= eng%n .or. .not. allocated(a%row_ptr) .or. .not. allocated(a%values)) then
       print *, "engine_set_hermitian: the matrix must be of order ", eng%n / 2, " (the engine's real order is ", eng%n, ")"
       error stop
    end if
    if (size(a%values) > 0) then
       call c_f_pointer(c_loc(a%values), pairs, [2 * size(a%values)])          ! the (re, im) pairs where they lie
       call check_dav(davh_set_operator_csr(eng%h, int(which - 1, c_int), a%row_ptr, a%col_idx, pairs, 1_c_int, tri), &
            "davh_set_operator_csr")
    else
       nothing = 0.0_dp
       call check_dav(davh_set_operator_csr(eng%h, int(which - 1, c_int), a%row_ptr, [0_c_int32_t], nothing, 1_c_int, tri), &
            "davh_set_operator_csr")
    end if
    if (which == 1) eng%free_semantics = .false.
  end subroutine engine_set_hermitian

  !> The same from a complex CSR matrix of order n (the engine's real order is 2 n) whose arrays are DEVICE memory of the engine's
  !> device - vals an array of complex(c_double_complex) - built on the GPU by davh_set_operator_csr_dev, bit for bit as
  !> engine_set_hermitian builds it.  base: 1 (default) or 0; lower: only the entries with column <= row are given; row_ptr_bits /
  !> col_bits: 64 (default for row_ptr) or 32 (default for col_idx).  The arrays must be complete when the call is made and are free
  !> again when it returns.  stat present: a refused matrix returns its non-zero status here (dav_last_error says why; the operator is
  !> left unset), otherwise the program stops.
  subroutine engine_set_hermitian_device(eng, which, n, row_ptr, col_idx, vals, base, lower, row_ptr_bits, col_bits, stat)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which, n
    type(c_ptr), intent(in) :: row_ptr, col_idx, vals
    integer, intent(in), optional :: base, row_ptr_bits, col_bits
    logical, intent(in), optional :: lower
    integer, intent(out), optional :: stat
    integer(c_int) :: ib, rb, cb, tri, ierr
    if (2 * n /= eng%n) then
       if (present(stat)) then
          stat = -1
          return
       end if
       print *, "engine_set_hermitian_device: the matrix must be of order ", eng%n / 2
       error stop
    end if
    ib = 1_c_int
    rb = 64_c_int
    cb = 32_c_int
    tri = DAV_CSR_FULL
    if (present(base)) ib = int(base, c_int)
    if (present(row_ptr_bits)) rb = int(row_ptr_bits, c_int)
    if (present(col_bits)) cb = int(col_bits, c_int)
    if (present(lower)) then
       if (lower) tri = DAV_CSR_LOWER
    end if
    ierr = davh_set_operator_csr_dev(eng%h, int(which - 1, c_int), row_ptr, rb, col_idx, cb, vals, ib, tri)
    if (present(stat)) then
       stat = int(ierr)
    else
       call check_dav(ierr, "davh_set_operator_csr_dev")
    end if
    if (ierr == 0 .and. which == 1) eng%free_semantics = .false.
  end subroutine engine_set_hermitian_device

  !> New values of a Hermitian operator set after engine_keep_value_map(eng, which, .true.): values has the length and order of the
  !> values of the set call and is read where it lies.  The pattern is not touched; values, diagonal, applies and solves equal bit for
  !> bit what a fresh engine_set_hermitian with these values gives.  (From device memory: engine_update_sparse_values_device of module
  !> davidson_sparse, with vals the complex device array of the set call.)
  subroutine engine_update_hermitian_values(eng, which, values)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    complex(dp), intent(in), contiguous, target :: values(:)
    real(dp), pointer :: pairs(:)
    real(dp) :: nothing(2)
    if (size(values) > 0) then
       call c_f_pointer(c_loc(values), pairs, [2 * size(values)])
       call check_dav(dav_update_operator_values(eng%h, int(which - 1, c_int), pairs), "dav_update_operator_values")
    else
       nothing = 0.0_dp
       call check_dav(dav_update_operator_values(eng%h, int(which - 1, c_int), nothing), "dav_update_operator_values")
    end if
  end subroutine engine_update_hermitian_values

  !> y = S x for a zcsr_matrix S (honouring lower) and a block x of complex columns
  subroutine zcsr_apply(s, x, y)
    type(zcsr_matrix), intent(in) :: s
    complex(dp), intent(in) :: x(:, :)
    complex(dp), intent(out) :: y(:, :)
    integer :: i, j
    integer(c_int64_t) :: p
    y = (0.0_dp, 0.0_dp)
    do i = 1, s%n
       do p = s%row_ptr(i), s%row_ptr(i + 1) - 1
          j = s%col_idx(p)
          y(i, :) = y(i, :) + s%values(p) * x(j, :)
          if (s%lower .and. j /= i) y(j, :) = y(j, :) + conjg(s%values(p)) * x(i, :)
       end do
    end do
  end subroutine zcsr_apply

  !> all eigenpairs of the Hermitian matrix a (overwritten by the vectors), ascending
  subroutine heev(a, w)
    complex(dp), intent(inout) :: a(:, :)
    real(dp), intent(out) :: w(:)
    complex(dp), allocatable :: work(:)
    real(dp), allocatable :: rwork(:)
    complex(dp) :: query(1)
    integer :: m, info
    m = size(a, 1)
    allocate(rwork(max(1, 3 * m - 2)))
    call zheev("V", "U", m, a, m, w, query, -1, rwork, info)
    allocate(work(max(1, int(query(1)))))
    call zheev("V", "U", m, a, m, w, work, size(work), rwork, info)
    if (info /= 0) then
       print *, "hermitian_eigenpairs: zheev failed with info = ", info
       error stop
    end if
  end subroutine heev

  !> The `lowest` complex eigenpairs (lambda ascending, x of shape (n, lowest) with x^H S x = I) of H x = lambda S x from the
  !> 2 * lowest real Ritz pairs of its real form: theta ascending, v of shape (2 n, 2 * lowest), S-orthonormal in the real form.
  !> b: the matrix S of a generalized problem (absent: S = I).  The real form has every eigenvalue twice and the solver leaves an
  !> arbitrary rotation inside each pair, so the columns z = v(odd rows) + i v(even rows) span a complex space of dimension `lowest`
  !> only: their Gram matrix G = z^H S z = I + i K (K real antisymmetric) has the eigenvalues 1 +- s in pairs, the `lowest` largest are
  !> >= 1 also where the cut goes through a degenerate cluster, and their vectors give an S-orthonormal basis z C of that space.  The
  !> Rayleigh quotient T = C^H (G diag(theta)) C on it, hermitised, has the eigenpairs (lambda, W); x = z C W.  O(n lowest^2) host work.
  subroutine hermitian_eigenpairs(theta, v, lowest, lambda, x, b)
    real(dp), intent(in) :: theta(:)
    real(dp), intent(in) :: v(:, :)
    integer, intent(in) :: lowest
    real(dp), intent(out) :: lambda(lowest)
    complex(dp), intent(out) :: x(:, :)
    type(zcsr_matrix), intent(in), optional :: b
    complex(dp), allocatable :: z(:, :), sz(:, :), g(:, :), u(:, :), c(:, :), t(:, :), gd(:, :)
    real(dp), allocatable :: gw(:), tw(:)
    integer :: n, m, j
    n = size(v, 1) / 2
    m = 2 * lowest
    if (size(v, 1) /= 2 * n .or. size(v, 2) < m .or. size(theta) < m .or. size(x, 1) /= n .or. size(x, 2) < lowest) then
       print *, "hermitian_eigenpairs: theta(2 * lowest), v(2 n, 2 * lowest) and x(n, lowest) are needed"
       error stop
    end if
    allocate(z(n, m), sz(n, m), g(m, m), u(m, m), gd(m, m), gw(m), c(m, lowest), t(lowest, lowest), tw(lowest))
    z = cmplx(v(1:2 * n - 1:2, 1:m), v(2:2 * n:2, 1:m), dp)
    if (present(b)) then
       call zcsr_apply(b, z, sz)
    else
       sz = z
    end if
    g = matmul(conjg(transpose(z)), sz)
    g = 0.5_dp * (g + conjg(transpose(g)))
    u = g
    call heev(u, gw)
    do j = 1, lowest
       c(:, j) = u(:, lowest + j) / sqrt(gw(lowest + j))
    end do
    do j = 1, m
       gd(:, j) = g(:, j) * theta(j)
    end do
    t = matmul(conjg(transpose(c)), matmul(gd, c))
    t = 0.5_dp * (t + conjg(transpose(t)))
    call heev(t, tw)
    lambda = tw
    x(:, 1:lowest) = matmul(z, matmul(c, t))
  end subroutine hermitian_eigenpairs

end module davidson_hermitian
