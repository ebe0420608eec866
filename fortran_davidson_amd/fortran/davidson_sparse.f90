!> Sparse operators: a symmetric real matrix in CSR (compressed sparse row) or BSR (block sparse row) form, 1-based as Fortran numbers
!> rows and columns, and engine_set_sparse, which hands either to a device-resident problem (dav_set_operator_csr / dav_set_operator_bsr,
!> include/davidson_hip.h); engine_set_sparse_device / engine_set_block_sparse_device take the same matrices from device arrays.  The solves of a csr_matrix / bsr_matrix are the specifics generalized_eigensolver_sparse /
!> generalized_eigensolver_bsr of the generic generalized_eigensolver (module davidson).  A coo_matrix holds the same matrix as unordered
!> (row, column, value) triples, duplicates included (davx_set_operator_coo); engine_set_coo_device takes the triples from device arrays.
module davidson_sparse
  use, intrinsic :: iso_c_binding
  use numeric_kinds, only: dp
  use davidson_hip_c
  use davidson_engine_setup, only: davidson_engine
  implicit none
  private
  public :: csr_matrix, bsr_matrix, engine_set_sparse, engine_set_sparse_device, engine_set_block_sparse_device
  public :: coo_matrix, engine_set_coo_device
  public :: engine_keep_value_map, engine_update_sparse_values, engine_update_sparse_values_device

  !> A symmetric real matrix of order n in CSR form, 1-based: the entries of row i are col_idx / values(row_ptr(i) : row_ptr(i+1) - 1).
  !> lower = .true.: only the entries with column <= row are given (the engine mirrors the strict lower part); .false.: every nonzero
  !> is given, and the matrix being symmetric is the caller's promise, as for a dense matrix.
  !> diagonals = .true. (DAV_CSR_DIAGONALS): the engine stores the matrix by its diagonals - for stencils, banded and tight-binding
  !> matrices; it refuses one with too many diagonals for its entries (nd * n > 4 * max(entries, n)), it never falls back to CSR.
  type :: csr_matrix
     integer :: n = 0
     integer(c_int64_t), allocatable :: row_ptr(:)
     integer(c_int32_t), allocatable :: col_idx(:)
     real(dp), allocatable :: values(:)
     logical :: lower = .false.
     logical :: diagonals = .false.
  end type csr_matrix

  !> csr_matrix(n, row_ptr, col_idx, values [, lower] [, diagonals]) from default-kind integer arrays, 1-based
  interface csr_matrix
     module procedure new_csr_matrix
  end interface csr_matrix

  !> A symmetric real matrix of order n as COO triples, 1-based: entry p is values(p) at (row_idx(p), col_idx(p)).  The triples may come
  !> in any order and may repeat a position: duplicates stay separate terms, in the order of p.  The operator built is, bit for bit,
  !> that of the csr_matrix obtained by a stable sort of the triples by row.  lower and diagonals: as for csr_matrix.
  type :: coo_matrix
     integer :: n = 0
     integer(c_int32_t), allocatable :: row_idx(:)
     integer(c_int32_t), allocatable :: col_idx(:)
     real(dp), allocatable :: values(:)
     logical :: lower = .false.
     logical :: diagonals = .false.
  end type coo_matrix

  !> coo_matrix(n, row_idx, col_idx, values [, lower] [, diagonals]) from default-kind integer arrays, 1-based
  interface coo_matrix
     module procedure new_coo_matrix
  end interface coo_matrix

  !> A symmetric real matrix of order n in BSR form with square blocks of a uniform size block_size = b (1..16, n a multiple of b),
  !> 1-based: the blocks of block row I are col_idx / values(:, :, row_ptr(I) : row_ptr(I+1) - 1), values(m, k, p) the entry (m, k) of
  !> block p.  lower = .true.: only the blocks with block column <= block row are given (a diagonal block in full; the engine mirrors
  !> the strict lower blocks); .false.: every nonzero block is given, and the symmetry is the caller's promise.
  type :: bsr_matrix
     integer :: n = 0
     integer :: block_size = 0
     integer(c_int64_t), allocatable :: row_ptr(:)
     integer(c_int32_t), allocatable :: col_idx(:)
     real(dp), allocatable :: values(:, :, :)
     logical :: lower = .false.
  end type bsr_matrix

  !> bsr_matrix(n, b, row_ptr, col_idx, values [, lower]) from default-kind integer arrays, 1-based
  interface bsr_matrix
     module procedure new_bsr_matrix
  end interface bsr_matrix

  !> engine_set_sparse(eng, which, a) with a csr_matrix, a bsr_matrix or a coo_matrix
  interface engine_set_sparse
     module procedure engine_set_sparse_csr
     module procedure engine_set_sparse_bsr
     module procedure engine_set_sparse_coo
  end interface engine_set_sparse

  !> engine_update_sparse_values(eng, which, values): new values on the kept pattern of a sparse operator set after
  !> engine_keep_value_map(eng, which, .true.) - values(:) as the values of the csr_matrix (or of the device array) of that set call,
  !> values(b, b, nnzb) as those of the bsr_matrix
  interface engine_update_sparse_values
     module procedure engine_update_sparse_values_csr
     module procedure engine_update_sparse_values_bsr
  end interface engine_update_sparse_values

contains

  !> Sticky switch of operator A (which = 1), B (which = 2) or the preconditioner M (which = 3): with on = .true. the NEXT engine_set_sparse / engine_set_sparse_device /
  !> engine_set_block_sparse_device call for that operator also keeps where every stored value came from (8 bytes per entry or block of
  !> this rank, 16 per row or block row of the matrix), so that engine_update_sparse_values can move new numbers into the kept pattern.
  !> It has no effect on an operator that is already set.
  subroutine engine_keep_value_map(eng, which, on)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    logical, intent(in) :: on
    call check_dav(dav_keep_value_map(eng%h, int(which - 1, c_int), merge(1_c_int, 0_c_int, on)), "dav_keep_value_map")
  end subroutine engine_keep_value_map

  !> New values of operator A (which = 1), B (which = 2) or the preconditioner M (which = 3), a sparse operator set after engine_keep_value_map: values has the length and
  !> order of the values of the set call (for a BSR operator its blocks one after the other, each as the set call had them).  The
  !> pattern is not touched; values, diagonal, applies and solves equal bit for bit what a fresh engine_set_sparse with these values
  !> gives.  The array is free again when the call returns.
  subroutine engine_update_sparse_values_csr(eng, which, values)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    real(dp), intent(in) :: values(:)
    real(dp) :: nothing(1)
    if (size(values) > 0) then
       call check_dav(dav_update_operator_values(eng%h, int(which - 1, c_int), values), "dav_update_operator_values")
    else
       nothing = 0.0_dp
       call check_dav(dav_update_operator_values(eng%h, int(which - 1, c_int), nothing), "dav_update_operator_values")
    end if
  end subroutine engine_update_sparse_values_csr

  !> The same for a BSR operator set from a bsr_matrix: values(m, k, p) the entry (m, k) of block p, as bsr_matrix has them
  subroutine engine_update_sparse_values_bsr(eng, which, values)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    real(dp), intent(in) :: values(:, :, :)
    real(dp) :: nothing(1)
    if (size(values) > 0) then
       call check_dav(dav_update_operator_values(eng%h, int(which - 1, c_int), values), "dav_update_operator_values")
    else
       nothing = 0.0_dp
       call check_dav(dav_update_operator_values(eng%h, int(which - 1, c_int), nothing), "dav_update_operator_values")
    end if
  end subroutine engine_update_sparse_values_bsr

  !> The same from DEVICE memory of the engine's device (vals as the vals of engine_set_sparse_device /
  !> engine_set_block_sparse_device, complete when the call is made and free again when it returns).  stat present: a refused update
  !> returns its non-zero status here (dav_last_error says why; the operator keeps its old values), otherwise the program stops.
  subroutine engine_update_sparse_values_device(eng, which, vals, stat)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    type(c_ptr), intent(in) :: vals
    integer, intent(out), optional :: stat
    integer(c_int) :: ierr
    ierr = dav_update_operator_values_dev(eng%h, int(which - 1, c_int), vals)
    if (present(stat)) then
       stat = int(ierr)
    else
       call check_dav(ierr, "dav_update_operator_values_dev")
    end if
  end subroutine engine_update_sparse_values_device

  function new_csr_matrix(n, row_ptr, col_idx, values, lower, diagonals) result(a)
    integer, intent(in) :: n
    integer, intent(in) :: row_ptr(:), col_idx(:)
    real(dp), intent(in) :: values(:)
    logical, intent(in), optional :: lower, diagonals
    type(csr_matrix) :: a
    if (size(row_ptr) /= n + 1) then
       print *, "csr_matrix: row_ptr must hold n + 1 = ", n + 1, " offsets, not ", size(row_ptr)
       error stop
    end if
    if (size(col_idx) < row_ptr(n + 1) - 1 .or. size(values) < row_ptr(n + 1) - 1) then
       print *, "csr_matrix: row_ptr(n + 1) - 1 = ", row_ptr(n + 1) - 1, " entries, but col_idx / values hold ", size(col_idx), &
            " / ", size(values)
       error stop
    end if
    a%n = n
    a%row_ptr = int(row_ptr, c_int64_t)
    a%col_idx = int(col_idx, c_int32_t)
    a%values = values
    if (present(lower)) a%lower = lower
    if (present(diagonals)) a%diagonals = diagonals
  end function new_csr_matrix

  !> Operator A (which = 1), B (which = 2) or the preconditioner M (which = 3) of the engine from a csr_matrix: the engine keeps the rows of its slab in HBM and applies
  !> them with its own CSR kernel.  The matrix is not referenced after the call.
  subroutine engine_set_sparse_csr(eng, which, a)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    type(csr_matrix), intent(in) :: a
    real(dp) :: nothing(1)
    integer(c_int) :: tri
    tri = merge(DAV_CSR_LOWER, DAV_CSR_FULL, a%lower)
    if (a%diagonals) tri = ior(tri, DAV_CSR_DIAGONALS)
    if (a%n /= eng%n .or. .not. allocated(a%row_ptr)) then
       print *, "engine_set_sparse: the matrix must be of order ", eng%n
       error stop
    end if
    if (size(a%values) > 0) then
       call check_dav(dav_set_operator_csr(eng%h, int(which - 1, c_int), a%row_ptr, a%col_idx, a%values, 1_c_int, tri), &
            "dav_set_operator_csr")
    else
       nothing = 0.0_dp
       call check_dav(dav_set_operator_csr(eng%h, int(which - 1, c_int), a%row_ptr, [0_c_int32_t], nothing, 1_c_int, tri), &
            "dav_set_operator_csr")
    end if
    ! a stored matrix: the dense driver's sticky convergence flags, as for engine_set_dense
    if (which == 1) eng%free_semantics = .false.
  end subroutine engine_set_sparse_csr

  !> Operator A (which = 1), B (which = 2) or the preconditioner M (which = 3) of the engine from a CSR matrix of order n whose arrays are DEVICE memory of the engine's
  !> device (hipfort, OpenMP offload, a GPU assembly stage): dav_set_operator_csr_dev builds the operator on the GPU, bit for bit as
  !> engine_set_sparse builds it from a csr_matrix holding the same arrays.  base: 1 (default, Fortran numbering) or 0; lower: only the
  !> entries with column <= row are given; row_ptr_bits / col_bits: 64 (default for row_ptr) or 32 (default for col_idx).  The arrays
  !> must be complete when the call is made (a caller that writes them asynchronously synchronises first) and are free again when it
  !> returns.  stat present: a refused matrix returns its non-zero status here (dav_last_error says why; the operator is left unset),
  !> otherwise the program stops.  diagonals = .true.: the matrix is stored by its diagonals, as for a csr_matrix with that component.
  subroutine engine_set_sparse_device(eng, which, n, row_ptr, col_idx, vals, base, lower, row_ptr_bits, col_bits, stat, diagonals)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which, n
    type(c_ptr), intent(in) :: row_ptr, col_idx, vals
    integer, intent(in), optional :: base, row_ptr_bits, col_bits
    logical, intent(in), optional :: lower
    integer, intent(out), optional :: stat
    logical, intent(in), optional :: diagonals
    integer(c_int) :: ib, rb, cb, tri, ierr
    if (n /= eng%n) then
       if (present(stat)) then
          stat = -1
          return
       end if
       print *, "engine_set_sparse_device: the matrix must be of order ", eng%n
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
    if (present(diagonals)) then
       if (diagonals) tri = ior(tri, DAV_CSR_DIAGONALS)
    end if
    ierr = dav_set_operator_csr_dev(eng%h, int(which - 1, c_int), row_ptr, rb, col_idx, cb, vals, ib, tri)
    if (present(stat)) then
       stat = int(ierr)
    else
       call check_dav(ierr, "dav_set_operator_csr_dev")
    end if
    if (ierr == 0 .and. which == 1) eng%free_semantics = .false.
  end subroutine engine_set_sparse_device

  function new_coo_matrix(n, row_idx, col_idx, values, lower, diagonals) result(a)
    integer, intent(in) :: n
    integer, intent(in) :: row_idx(:), col_idx(:)
    real(dp), intent(in) :: values(:)
    logical, intent(in), optional :: lower, diagonals
    type(coo_matrix) :: a
    if (size(row_idx) /= size(values) .or. size(col_idx) /= size(values)) then
       print *, "coo_matrix: row_idx / col_idx / values hold ", size(row_idx), " / ", size(col_idx), " / ", size(values), &
            " triples: the three must be of one length"
       error stop
    end if
    a%n = n
    a%row_idx = int(row_idx, c_int32_t)
    a%col_idx = int(col_idx, c_int32_t)
    a%values = values
    if (present(lower)) a%lower = lower
    if (present(diagonals)) a%diagonals = diagonals
  end function new_coo_matrix

  !> Operator A (which = 1), B (which = 2) or the preconditioner M (which = 3) of the engine from a coo_matrix: the operator of the
  !> csr_matrix that a stable sort of the triples by row gives, bit for bit.  After engine_keep_value_map,
  !> engine_update_sparse_values takes the values in the order of the triples.  The matrix is not referenced after the call.
  subroutine engine_set_sparse_coo(eng, which, a)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    type(coo_matrix), intent(in) :: a
    real(dp) :: nothing(1)
    integer(c_int) :: tri
    tri = merge(DAV_CSR_LOWER, DAV_CSR_FULL, a%lower)
    if (a%diagonals) tri = ior(tri, DAV_CSR_DIAGONALS)
    if (a%n /= eng%n .or. .not. allocated(a%values)) then
       print *, "engine_set_sparse: the matrix must be of order ", eng%n
       error stop
    end if
    if (size(a%values) > 0) then
       call check_dav(davx_set_operator_coo(eng%h, int(which - 1, c_int), int(size(a%values), c_int64_t), a%row_idx, a%col_idx, &
            a%values, 1_c_int, tri), "davx_set_operator_coo")
    else
       nothing = 0.0_dp
       call check_dav(davx_set_operator_coo(eng%h, int(which - 1, c_int), 0_c_int64_t, [0_c_int32_t], [0_c_int32_t], nothing, 1_c_int, &
            tri), "davx_set_operator_coo")
    end if
    if (which == 1) eng%free_semantics = .false.
  end subroutine engine_set_sparse_coo

  !> Operator A (which = 1), B (which = 2) or the preconditioner M (which = 3) of the engine from nnz COO triples of a matrix of order
  !> n whose arrays are DEVICE memory of the engine's device: davx_set_operator_coo_dev builds the operator on the GPU, bit for bit as
  !> engine_set_sparse builds it from a coo_matrix holding the same triples.  base: 1 (default) or 0; lower: only entries with column
  !> <= row are given; row_bits / col_bits: 32 (default) or 64.  The arrays must be complete when the call is made and are free again
  !> when it returns.  stat present: a refused matrix returns its non-zero status here (dav_last_error says why; the operator is left
  !> unset), otherwise the program stops.  diagonals = .true.: the matrix is stored by its diagonals.
  subroutine engine_set_coo_device(eng, which, n, nnz, row_idx, col_idx, vals, base, lower, row_bits, col_bits, stat, diagonals)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which, n
    integer(c_int64_t), intent(in) :: nnz
    type(c_ptr), intent(in) :: row_idx, col_idx, vals
    integer, intent(in), optional :: base, row_bits, col_bits
    logical, intent(in), optional :: lower
    integer, intent(out), optional :: stat
    logical, intent(in), optional :: diagonals
    integer(c_int) :: ib, rb, cb, tri, ierr
    if (n /= eng%n) then
       if (present(stat)) then
          stat = -1
          return
       end if
       print *, "engine_set_coo_device: the matrix must be of order ", eng%n
       error stop
    end if
    ib = 1_c_int
    rb = 32_c_int
    cb = 32_c_int
    tri = DAV_CSR_FULL
    if (present(base)) ib = int(base, c_int)
    if (present(row_bits)) rb = int(row_bits, c_int)
    if (present(col_bits)) cb = int(col_bits, c_int)
    if (present(lower)) then
       if (lower) tri = DAV_CSR_LOWER
    end if
    if (present(diagonals)) then
       if (diagonals) tri = ior(tri, DAV_CSR_DIAGONALS)
    end if
    ierr = davx_set_operator_coo_dev(eng%h, int(which - 1, c_int), nnz, row_idx, rb, col_idx, cb, vals, ib, tri)
    if (present(stat)) then
       stat = int(ierr)
    else
       call check_dav(ierr, "davx_set_operator_coo_dev")
    end if
    if (ierr == 0 .and. which == 1) eng%free_semantics = .false.
  end subroutine engine_set_coo_device

  function new_bsr_matrix(n, b, row_ptr, col_idx, values, lower) result(a)
    integer, intent(in) :: n, b
    integer, intent(in) :: row_ptr(:), col_idx(:)
    real(dp), intent(in) :: values(:, :, :)
    logical, intent(in), optional :: lower
    type(bsr_matrix) :: a
    integer :: nb
    if (b < 1 .or. b > 16) then
       print *, "bsr_matrix: block size ", b, " must lie in 1..16"
       error stop
    end if
    if (mod(n, b) /= 0) then
       print *, "bsr_matrix: n = ", n, " is not a multiple of the block size ", b
       error stop
    end if
    nb = n / b
    if (size(row_ptr) /= nb + 1) then
       print *, "bsr_matrix: row_ptr must hold n / b + 1 = ", nb + 1, " offsets, not ", size(row_ptr)
       error stop
    end if
    if (size(values, 1) /= b .or. size(values, 2) /= b) then
       print *, "bsr_matrix: values must have the shape (b, b, nnzb)"
       error stop
    end if
    if (size(col_idx) < row_ptr(nb + 1) - 1 .or. size(values, 3) < row_ptr(nb + 1) - 1) then
       print *, "bsr_matrix: row_ptr(n / b + 1) - 1 = ", row_ptr(nb + 1) - 1, " blocks, but col_idx / values hold ", size(col_idx), &
            " / ", size(values, 3)
       error stop
    end if
    a%n = n
    a%block_size = b
    a%row_ptr = int(row_ptr, c_int64_t)
    a%col_idx = int(col_idx, c_int32_t)
    a%values = values
    if (present(lower)) a%lower = lower
  end function new_bsr_matrix

  !> Operator A (which = 1), B (which = 2) or the preconditioner M (which = 3) of the engine from a bsr_matrix: the engine keeps the block rows of its slab in HBM and
  !> applies them with its own matrix-core BSR kernel.  The matrix is not referenced after the call.
  subroutine engine_set_sparse_bsr(eng, which, a)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    type(bsr_matrix), intent(in) :: a
    real(dp) :: nothing(1)
    if (a%n /= eng%n .or. .not. allocated(a%row_ptr) .or. .not. allocated(a%values)) then
       print *, "engine_set_sparse: the matrix must be of order ", eng%n
       error stop
    end if
    if (size(a%values) > 0) then
       call check_dav(dav_set_operator_bsr(eng%h, int(which - 1, c_int), int(a%block_size, c_int), a%row_ptr, a%col_idx, a%values, &
            1_c_int, merge(DAV_CSR_LOWER, DAV_CSR_FULL, a%lower), DAV_BSR_COL_MAJOR), "dav_set_operator_bsr")
    else
       nothing = 0.0_dp
       call check_dav(dav_set_operator_bsr(eng%h, int(which - 1, c_int), int(a%block_size, c_int), a%row_ptr, [0_c_int32_t], nothing, &
            1_c_int, merge(DAV_CSR_LOWER, DAV_CSR_FULL, a%lower), DAV_BSR_COL_MAJOR), "dav_set_operator_bsr")
    end if
    if (which == 1) eng%free_semantics = .false.
  end subroutine engine_set_sparse_bsr

  !> Operator A (which = 1), B (which = 2) or the preconditioner M (which = 3) of the engine from a BSR matrix of order n with square blocks of size block_size whose
  !> arrays are DEVICE memory of the engine's device: dav_set_operator_bsr_dev builds the operator on the GPU, bit for bit as
  !> engine_set_sparse builds it from a bsr_matrix holding the same arrays.  base: 1 (default, Fortran numbering of block rows and
  !> columns) or 0; lower: only the blocks with block column <= block row are given; row_major: the b * b values of a block are in C
  !> order (default .false.: a Fortran values(b, b, nnzb)); row_ptr_bits / col_bits: 64 (default for row_ptr) or 32 (default for
  !> col_idx).  The arrays must be complete when the call is made and are free again when it returns.  stat present: a refused matrix
  !> returns its non-zero status here (dav_last_error says why; the operator is left unset), otherwise the program stops.
  subroutine engine_set_block_sparse_device(eng, which, n, block_size, row_ptr, col_idx, vals, base, lower, row_major, row_ptr_bits, &
       col_bits, stat)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which, n, block_size
    type(c_ptr), intent(in) :: row_ptr, col_idx, vals
    integer, intent(in), optional :: base, row_ptr_bits, col_bits
    logical, intent(in), optional :: lower, row_major
    integer, intent(out), optional :: stat
    integer(c_int) :: ib, rb, cb, tri, lay, ierr
    if (n /= eng%n) then
       if (present(stat)) then
          stat = -1
          return
       end if
       print *, "engine_set_block_sparse_device: the matrix must be of order ", eng%n
       error stop
    end if
    ib = 1_c_int
    rb = 64_c_int
    cb = 32_c_int
    tri = DAV_CSR_FULL
    lay = DAV_BSR_COL_MAJOR
    if (present(base)) ib = int(base, c_int)
    if (present(row_ptr_bits)) rb = int(row_ptr_bits, c_int)
    if (present(col_bits)) cb = int(col_bits, c_int)
    if (present(lower)) then
       if (lower) tri = DAV_CSR_LOWER
    end if
    if (present(row_major)) then
       if (row_major) lay = DAV_BSR_ROW_MAJOR
    end if
    ierr = dav_set_operator_bsr_dev(eng%h, int(which - 1, c_int), int(block_size, c_int), row_ptr, rb, col_idx, cb, vals, ib, tri, lay)
    if (present(stat)) then
       stat = int(ierr)
    else
       call check_dav(ierr, "dav_set_operator_bsr_dev")
    end if
    if (ierr == 0 .and. which == 1) eng%free_semantics = .false.
  end subroutine engine_set_block_sparse_device

end module davidson_sparse
