!> bind(C) doors into the Fortran API so that non-Fortran callers (the pytest suite and bench.py
!> through ctypes) exercise exactly what a Fortran user calls: `generalized_eigensolver` of module
!> `davidson` and the helper modules.  Nothing here computes; it only forwards.
module davidson_c_api
  use, intrinsic :: iso_c_binding
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver
  use davidson_method, only: method_label
  use davidson_device
  use davidson_free, only: free_matmul
  use davidson_sparse, only: csr_matrix, bsr_matrix, engine_set_sparse, engine_set_sparse_device, engine_set_block_sparse_device, &
       coo_matrix, engine_set_coo_device, engine_keep_value_map, engine_update_sparse_values, engine_update_sparse_values_device
  use davidson_hermitian, only: engine_set_hermitian_device
  use davidson_hip_c, only: DAV_CSR_LOWER, DAV_CSR_DIAGONALS, DAV_BSR_ROW_MAJOR, DAV_BSR_COL_MAJOR, dav_set_operator_bsr_dev, davh_set_operator_csr, check_dav
  use lapack_wrapper
  use array_utils
  implicit none

  abstract interface
     subroutine c_block_apply(n, k, x, y) bind(C)
       import :: c_int, c_double
       integer(c_int), value :: n, k
       real(c_double), intent(in) :: x(n, k)
       real(c_double), intent(out) :: y(n, k)
     end subroutine c_block_apply
  end interface
  procedure(c_block_apply), pointer, save :: cb_a => null(), cb_b => null()

contains

  ! The solve doors.  max_dim < 0: max_dim_sub is absent; has_b = 0: second_matrix is absent - an unallocated allocatable and a
  ! disassociated pointer are absent optional arguments (Fortran 2008), so each body calls generalized_eigensolver once per specific:
  ! the reference's argument list, and with x0 present the one with initial_vectors=.

  !> the body of fd_dense_solve and fd_dense_solve_guess (x0 present)
  subroutine dense_solve(n, a, has_b, b, lowest, method, max_it, tol, max_dim, evals, evecs, iters, x0)
    integer(c_int), intent(in) :: n, has_b, lowest, method, max_it, max_dim
    real(c_double), intent(in) :: tol
    real(c_double), intent(in), target :: a(n, n), b(n, *)
    real(c_double), intent(out) :: evals(lowest), evecs(n, lowest)
    integer(c_int), intent(out) :: iters
    real(c_double), intent(in), optional :: x0(:, :)
    integer, allocatable :: md
    real(c_double), pointer :: bp(:, :)
    integer :: it
    if (max_dim >= 0) md = max_dim
    bp => null()
    if (has_b /= 0) bp => b(:, 1:n)
    if (present(x0)) then
       call generalized_eigensolver(a, evals, evecs, lowest, method_label(method), max_it, tol, it, md, bp, initial_vectors=x0)
    else
       call generalized_eigensolver(a, evals, evecs, lowest, method_label(method), max_it, tol, it, md, bp)
    end if
    iters = it
  end subroutine dense_solve

  !> generalized_eigensolver(matrix, ...) - dense specific
  subroutine fd_dense_solve(n, a, has_b, b, lowest, method, max_it, tol, max_dim, evals, evecs, iters) &
       bind(C, name="fd_dense_solve")
    integer(c_int), value :: n, has_b, lowest, method, max_it, max_dim
    real(c_double), value :: tol
    real(c_double), intent(in) :: a(n, n), b(n, *)
    real(c_double), intent(out) :: evals(lowest), evecs(n, lowest)
    integer(c_int), intent(out) :: iters
    call dense_solve(n, a, has_b, b, lowest, method, max_it, tol, max_dim, evals, evecs, iters)
  end subroutine fd_dense_solve

  !> A csr_matrix from C arrays (row_ptr: n + 1 int64 offsets, col_idx: int32) numbered from `base` (0 or 1): renumbered from 1.
  !> `lower` is the flag word of the CSR set entries: bit 0 = lower triangle, bit 1 = stored by diagonals (DAV_CSR_DIAGONALS)
  function csr_from_c(n, row_ptr, col_idx, vals, base, lower) result(a)
    integer(c_int), intent(in) :: n, base, lower
    integer(c_int64_t), intent(in) :: row_ptr(n + 1)
    integer(c_int32_t), intent(in) :: col_idx(*)
    real(c_double), intent(in) :: vals(*)
    type(csr_matrix) :: a
    integer(c_int64_t) :: nnz
    nnz = row_ptr(n + 1) - base
    a%n = n
    a%row_ptr = row_ptr + (1 - base)
    a%col_idx = col_idx(1:nnz) + int(1 - base, c_int32_t)
    a%values = vals(1:nnz)
    a%lower = iand(lower, DAV_CSR_LOWER) /= 0
    a%diagonals = iand(lower, DAV_CSR_DIAGONALS) /= 0
  end function csr_from_c

  !> the body of fd_sparse_solve and fd_sparse_solve_guess (x0 present); B has the base and the triangle of A
  subroutine sparse_solve(n, rp, col, vals, has_b, rpb, colb, valsb, base, lower, lowest, method, max_it, tol, max_dim, evals, evecs, &
       iters, x0)
    integer(c_int), intent(in) :: n, has_b, base, lower, lowest, method, max_it, max_dim
    integer(c_int64_t), intent(in) :: rp(n + 1), rpb(*)
    integer(c_int32_t), intent(in) :: col(*), colb(*)
    real(c_double), intent(in) :: vals(*), valsb(*), tol
    real(c_double), intent(out) :: evals(lowest), evecs(n, lowest)
    integer(c_int), intent(out) :: iters
    real(c_double), intent(in), optional :: x0(:, :)
    type(csr_matrix) :: a
    type(csr_matrix), allocatable :: b
    integer, allocatable :: md
    integer :: it
    if (max_dim >= 0) md = max_dim
    a = csr_from_c(n, rp, col, vals, base, lower)
    if (has_b /= 0) b = csr_from_c(n, rpb, colb, valsb, base, lower)
    if (present(x0)) then
       call generalized_eigensolver(a, evals, evecs, lowest, method_label(method), max_it, tol, it, md, b, initial_vectors=x0)
    else
       call generalized_eigensolver(a, evals, evecs, lowest, method_label(method), max_it, tol, it, md, b)
    end if
    iters = it
  end subroutine sparse_solve

  !> generalized_eigensolver(a_csr, ...) - sparse specific
  subroutine fd_sparse_solve(n, rp, col, vals, has_b, rpb, colb, valsb, base, lower, lowest, method, max_it, tol, max_dim, evals, &
       evecs, iters) bind(C, name="fd_sparse_solve")
    integer(c_int), value :: n, has_b, base, lower, lowest, method, max_it, max_dim
    integer(c_int64_t), intent(in) :: rp(n + 1), rpb(*)
    integer(c_int32_t), intent(in) :: col(*), colb(*)
    real(c_double), intent(in) :: vals(*), valsb(*)
    real(c_double), value :: tol
    real(c_double), intent(out) :: evals(lowest), evecs(n, lowest)
    integer(c_int), intent(out) :: iters
    call sparse_solve(n, rp, col, vals, has_b, rpb, colb, valsb, base, lower, lowest, method, max_it, tol, max_dim, evals, evecs, iters)
  end subroutine fd_sparse_solve

  !> A bsr_matrix from C arrays (row_ptr: n / b + 1 int64 offsets, col_idx: int32 block columns, vals: b * b values per block in
  !> Fortran order values(m, k, p)) numbered from `base` (0 or 1): renumbered from 1
  function bsr_from_c(n, b, row_ptr, col_idx, vals, base, lower) result(a)
    integer(c_int), intent(in) :: n, b, base, lower
    integer(c_int64_t), intent(in) :: row_ptr(n / b + 1)
    integer(c_int32_t), intent(in) :: col_idx(*)
    real(c_double), intent(in) :: vals(b, b, *)
    type(bsr_matrix) :: a
    integer(c_int64_t) :: nnzb
    if (iand(lower, DAV_CSR_DIAGONALS) /= 0) then
       print *, "bsr_matrix: DAV_CSR_DIAGONALS serves CSR matrices only - a BSR matrix is not stored by diagonals"
       error stop
    end if
    nnzb = row_ptr(n / b + 1) - base
    a%n = n
    a%block_size = b
    a%row_ptr = row_ptr + (1 - base)
    a%col_idx = col_idx(1:nnzb) + int(1 - base, c_int32_t)
    a%values = vals(:, :, 1:nnzb)
    a%lower = iand(lower, DAV_CSR_LOWER) /= 0
  end function bsr_from_c

  !> the body of fd_bsr_solve and fd_bsr_solve_guess (x0 present); B has the block size, the base and the triangle of A
  subroutine bsr_solve(n, b, rp, col, vals, has_b, rpb, colb, valsb, base, lower, lowest, method, max_it, tol, max_dim, evals, evecs, &
       iters, x0)
    integer(c_int), intent(in) :: n, b, has_b, base, lower, lowest, method, max_it, max_dim
    integer(c_int64_t), intent(in) :: rp(*), rpb(*)
    integer(c_int32_t), intent(in) :: col(*), colb(*)
    real(c_double), intent(in) :: vals(*), valsb(*), tol
    real(c_double), intent(out) :: evals(lowest), evecs(n, lowest)
    integer(c_int), intent(out) :: iters
    real(c_double), intent(in), optional :: x0(:, :)
    type(bsr_matrix) :: a
    type(bsr_matrix), allocatable :: bm
    integer, allocatable :: md
    integer :: it
    if (max_dim >= 0) md = max_dim
    a = bsr_from_c(n, b, rp, col, vals, base, lower)
    if (has_b /= 0) bm = bsr_from_c(n, b, rpb, colb, valsb, base, lower)
    if (present(x0)) then
       call generalized_eigensolver(a, evals, evecs, lowest, method_label(method), max_it, tol, it, md, bm, initial_vectors=x0)
    else
       call generalized_eigensolver(a, evals, evecs, lowest, method_label(method), max_it, tol, it, md, bm)
    end if
    iters = it
  end subroutine bsr_solve

  !> generalized_eigensolver(a_bsr, ...) - block-sparse specific
  subroutine fd_bsr_solve(n, b, rp, col, vals, has_b, rpb, colb, valsb, base, lower, lowest, method, max_it, tol, max_dim, evals, &
       evecs, iters) bind(C, name="fd_bsr_solve")
    integer(c_int), value :: n, b, has_b, base, lower, lowest, method, max_it, max_dim
    integer(c_int64_t), intent(in) :: rp(*), rpb(*)
    integer(c_int32_t), intent(in) :: col(*), colb(*)
    real(c_double), intent(in) :: vals(*), valsb(*)
    real(c_double), value :: tol
    real(c_double), intent(out) :: evals(lowest), evecs(n, lowest)
    integer(c_int), intent(out) :: iters
    call bsr_solve(n, b, rp, col, vals, has_b, rpb, colb, valsb, base, lower, lowest, method, max_it, tol, max_dim, evals, evecs, iters)
  end subroutine fd_bsr_solve

  function apply_cb_a(input_vect) result(output_vect)
    real(dp), dimension(:, :), intent(in) :: input_vect
    real(dp), dimension(size(input_vect, 1), size(input_vect, 2)) :: output_vect
    real(dp), allocatable :: x(:, :)
    x = input_vect
    call cb_a(int(size(x, 1), c_int), int(size(x, 2), c_int), x, output_vect)
  end function apply_cb_a

  function apply_cb_b(input_vect) result(output_vect)
    real(dp), dimension(:, :), intent(in) :: input_vect
    real(dp), dimension(size(input_vect, 1), size(input_vect, 2)) :: output_vect
    real(dp), allocatable :: x(:, :)
    x = input_vect
    call cb_b(int(size(x, 1), c_int), int(size(x, 2), c_int), x, output_vect)
  end function apply_cb_b

  !> the body of fd_free_solve and fd_free_solve_guess (x0 present)
  subroutine free_solve(fa, fb, n, lowest, max_it, tol, max_dim, evals, evecs, iters, x0)
    type(c_funptr), intent(in) :: fa, fb
    integer(c_int), intent(in) :: n, lowest, max_it, max_dim
    real(c_double), intent(in) :: tol
    real(c_double), intent(out) :: evals(lowest), evecs(n, lowest)
    integer(c_int), intent(out) :: iters
    real(c_double), intent(in), optional :: x0(:, :)
    integer :: it
    call c_f_procpointer(fa, cb_a)
    call c_f_procpointer(fb, cb_b)
    if (present(x0)) then
       call generalized_eigensolver(apply_cb_a, evals, evecs, lowest, "DPR", max_it, tol, it, max_dim, apply_cb_b, initial_vectors=x0)
    else
       call generalized_eigensolver(apply_cb_a, evals, evecs, lowest, "DPR", max_it, tol, it, max_dim, apply_cb_b)
    end if
    iters = it
  end subroutine free_solve

  !> generalized_eigensolver(fun_A, ..., fun_B) - matrix-free specific with C callbacks.
  subroutine fd_free_solve(n, fa, fb, lowest, max_it, tol, max_dim, evals, evecs, iters) bind(C, name="fd_free_solve")
    integer(c_int), value :: n, lowest, max_it, max_dim
    type(c_funptr), value :: fa, fb
    real(c_double), value :: tol
    real(c_double), intent(out) :: evals(lowest), evecs(n, lowest)
    integer(c_int), intent(out) :: iters
    call free_solve(fa, fb, n, lowest, max_it, tol, max_dim, evals, evecs, iters)
  end subroutine fd_free_solve

  ! ---- device-resident engine ---------------------------------------------------------------------
  function fd_engine_create(n, lowest, max_dim, gev, device, rank, nranks) result(p) bind(C, name="fd_engine_create")
    integer(c_int), value :: n, lowest, max_dim, gev, device, rank, nranks
    type(c_ptr) :: p
    type(davidson_engine), pointer :: eng
    integer, allocatable :: md                  ! max_dim < 0: max_dim_sub is absent
    allocate(eng)
    if (max_dim >= 0) md = max_dim
    call engine_create(eng, n, lowest, md, gev /= 0, device, rank, nranks)
    p = c_loc(eng)
  end function fd_engine_create

  subroutine fd_engine_destroy(p) bind(C, name="fd_engine_destroy")
    type(c_ptr), value :: p
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    call engine_destroy(eng)
    deallocate(eng)
  end subroutine fd_engine_destroy

  !> raw C handle (for dav_get_stats / dav_bench_apply from the harness)
  function fd_engine_handle(p) result(h) bind(C, name="fd_engine_handle")
    type(c_ptr), value :: p
    type(c_ptr) :: h
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    h = eng%h
  end function fd_engine_handle

  subroutine fd_engine_comm_unique_id(id) bind(C, name="fd_engine_comm_unique_id")
    character(kind=c_char), intent(out) :: id(128)
    call engine_comm_unique_id(id)
  end subroutine fd_engine_comm_unique_id

  subroutine fd_engine_comm_init(p, id) bind(C, name="fd_engine_comm_init")
    type(c_ptr), value :: p
    character(kind=c_char), intent(in) :: id(128)
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    call engine_comm_init(eng, id)
  end subroutine fd_engine_comm_init

  subroutine fd_engine_set_storage(p, mode) bind(C, name="fd_engine_set_storage")
    type(c_ptr), value :: p
    integer(c_int), value :: mode
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    if (mode == 1) then
       call engine_set_storage(eng, "symmetric")
    else
       call engine_set_storage(eng, "full")
    end if
  end subroutine fd_engine_set_storage

  subroutine fd_engine_set_inner_precision(p, bits) bind(C, name="fd_engine_set_inner_precision")
    type(c_ptr), value :: p
    integer(c_int), value :: bits
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    call engine_set_inner_precision(eng, int(bits))
  end subroutine fd_engine_set_inner_precision

  subroutine fd_engine_set_device_rr(p, on) bind(C, name="fd_engine_set_device_rr")
    type(c_ptr), value :: p
    integer(c_int), value :: on
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    call engine_set_device_rr(eng, on /= 0)
  end subroutine fd_engine_set_device_rr

  subroutine fd_engine_set_policy(p, code) bind(C, name="fd_engine_set_policy")
    type(c_ptr), value :: p
    integer(c_int), value :: code
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    if (code == 1) then
       call engine_set_correction_policy(eng, "unconverged")
    else if (code == 2) then
       call engine_set_correction_policy(eng, "locking")
    else
       call engine_set_correction_policy(eng, "all")
    end if
  end subroutine fd_engine_set_policy

  subroutine fd_engine_set_dense(p, which, a) bind(C, name="fd_engine_set_dense")
    type(c_ptr), value :: p
    integer(c_int), value :: which
    real(c_double), intent(in), target :: a(*)
    type(davidson_engine), pointer :: eng
    real(c_double), pointer :: mat(:, :)
    call c_f_pointer(p, eng)
    call c_f_pointer(c_loc(a), mat, [eng%n, eng%n])
    call engine_set_dense(eng, int(which), mat)
  end subroutine fd_engine_set_dense

  !> engine_set_sparse(eng, which, a) with a csr_matrix from C arrays numbered from `base`
  subroutine fd_engine_set_sparse(p, which, n, rp, col, vals, base, lower) bind(C, name="fd_engine_set_sparse")
    type(c_ptr), value :: p
    integer(c_int), value :: which, n, base, lower
    integer(c_int64_t), intent(in) :: rp(n + 1)
    integer(c_int32_t), intent(in) :: col(*)
    real(c_double), intent(in) :: vals(*)
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    call engine_set_sparse(eng, int(which), csr_from_c(n, rp, col, vals, base, lower))
  end subroutine fd_engine_set_sparse

  !> engine_set_sparse_device(eng, which, n, ...) with device arrays: returns the engine's status (0 = set; otherwise dav_last_error
  !> says why and the operator is unset) instead of stopping the process - device arrays cannot be checked on the host first
  function fd_engine_set_sparse_device(p, which, n, rp, rp_bits, col, col_bits, vals, base, lower) result(stat) &
       bind(C, name="fd_engine_set_sparse_device")
    type(c_ptr), value :: p
    integer(c_int), value :: which, n, rp_bits, col_bits, base, lower
    type(c_ptr), value :: rp, col, vals
    integer(c_int) :: stat
    type(davidson_engine), pointer :: eng
    integer :: st
    call c_f_pointer(p, eng)
    call engine_set_sparse_device(eng, int(which), int(n), rp, col, vals, base=int(base), lower=iand(lower, DAV_CSR_LOWER) /= 0, &
         row_ptr_bits=int(rp_bits), col_bits=int(col_bits), stat=st, diagonals=iand(lower, DAV_CSR_DIAGONALS) /= 0)
    stat = int(st, c_int)
  end function fd_engine_set_sparse_device

  !> engine_set_sparse(eng, which, a) with a coo_matrix from C arrays of nnz triples numbered from `base`: renumbered from 1
  subroutine fdx_engine_set_coo(p, which, n, nnz, row, col, vals, base, lower) bind(C, name="fdx_engine_set_coo")
    type(c_ptr), value :: p
    integer(c_int), value :: which, n, base, lower
    integer(c_int64_t), value :: nnz
    integer(c_int32_t), intent(in) :: row(*), col(*)
    real(c_double), intent(in) :: vals(*)
    type(davidson_engine), pointer :: eng
    type(coo_matrix) :: a
    call c_f_pointer(p, eng)
    a%n = int(n)
    a%row_idx = row(1:nnz) + (1_c_int32_t - base)
    a%col_idx = col(1:nnz) + (1_c_int32_t - base)
    a%values = vals(1:nnz)
    a%lower = iand(lower, DAV_CSR_LOWER) /= 0
    a%diagonals = iand(lower, DAV_CSR_DIAGONALS) /= 0
    call engine_set_sparse(eng, int(which), a)
  end subroutine fdx_engine_set_coo

  !> engine_set_coo_device(eng, which, n, nnz, ...) with device arrays of COO triples: returns the engine's status, as
  !> fd_engine_set_sparse_device does; `lower` is the same flag word
  function fdx_engine_set_coo_device(p, which, n, nnz, row, row_bits, col, col_bits, vals, base, lower) result(stat) &
       bind(C, name="fdx_engine_set_coo_device")
    type(c_ptr), value :: p
    integer(c_int), value :: which, n, row_bits, col_bits, base, lower
    integer(c_int64_t), value :: nnz
    type(c_ptr), value :: row, col, vals
    integer(c_int) :: stat
    type(davidson_engine), pointer :: eng
    integer :: st
    call c_f_pointer(p, eng)
    call engine_set_coo_device(eng, int(which), int(n), nnz, row, col, vals, base=int(base), lower=iand(lower, DAV_CSR_LOWER) /= 0, &
         row_bits=int(row_bits), col_bits=int(col_bits), stat=st, diagonals=iand(lower, DAV_CSR_DIAGONALS) /= 0)
    stat = int(st, c_int)
  end function fdx_engine_set_coo_device

  !> engine_set_hermitian for C arrays of a complex CSR matrix of order n (the engine's is 2 n) numbered from `base`; vals: 2 nnz
  !> doubles, (re, im) pairs.  The arrays go to davh_set_operator_csr as they are - no zcsr_matrix is built, the values are read where
  !> they lie, and the engine's messages count entries and rows from `base`.
  subroutine fdh_engine_set_hermitian(p, which, n, rp, col, vals, base, lower) bind(C, name="fdh_engine_set_hermitian")
    type(c_ptr), value :: p
    integer(c_int), value :: which, n, base, lower
    integer(c_int64_t), intent(in) :: rp(n + 1)
    integer(c_int32_t), intent(in) :: col(*)
    real(c_double), intent(in) :: vals(*)
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    if (2 * n /= eng%n) then
       print *, "fdh_engine_set_hermitian: the matrix must be of order ", eng%n / 2
       error stop
    end if
    call check_dav(davh_set_operator_csr(eng%h, which - 1_c_int, rp, col, vals, base, iand(lower, DAV_CSR_LOWER)), &
         "davh_set_operator_csr")
    if (which == 1) eng%free_semantics = .false.
  end subroutine fdh_engine_set_hermitian

  !> engine_set_hermitian_device(eng, which, n, ...) with device arrays: returns the engine's status, as fd_engine_set_sparse_device does
  function fdh_engine_set_hermitian_device(p, which, n, rp, rp_bits, col, col_bits, vals, base, lower) result(stat) &
       bind(C, name="fdh_engine_set_hermitian_device")
    type(c_ptr), value :: p
    integer(c_int), value :: which, n, rp_bits, col_bits, base, lower
    type(c_ptr), value :: rp, col, vals
    integer(c_int) :: stat
    type(davidson_engine), pointer :: eng
    integer :: st
    call c_f_pointer(p, eng)
    call engine_set_hermitian_device(eng, int(which), int(n), rp, col, vals, base=int(base), lower=iand(lower, DAV_CSR_LOWER) /= 0, &
         row_ptr_bits=int(rp_bits), col_bits=int(col_bits), stat=st)
    stat = int(st, c_int)
  end function fdh_engine_set_hermitian_device

  !> engine_build_preconditioner(eng, sigma, level, stat): returns the engine's status, as fd_engine_set_sparse_device does
  function fdp_engine_build_fsai(p, sigma, level) result(stat) bind(C, name="fdp_engine_build_fsai")
    type(c_ptr), value :: p
    real(c_double), value :: sigma
    integer(c_int), value :: level
    integer(c_int) :: stat
    type(davidson_engine), pointer :: eng
    integer :: st
    call c_f_pointer(p, eng)
    call engine_build_preconditioner(eng, sigma, int(level), st)
    stat = int(st, c_int)
  end function fdp_engine_build_fsai

  !> engine_preconditioner_info(eng, nnz, longest_row, longest_col)
  subroutine fdp_engine_fsai_info(p, nnz, longest_row, longest_col) bind(C, name="fdp_engine_fsai_info")
    type(c_ptr), value :: p
    integer(c_int64_t), intent(out) :: nnz, longest_row, longest_col
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    call engine_preconditioner_info(eng, nnz, longest_row, longest_col)
  end subroutine fdp_engine_fsai_info

  !> engine_build_block_preconditioner(eng, sigma, level, stat): returns the engine's status, as fd_engine_set_sparse_device does
  function fdq_engine_build_block_fsai(p, sigma, level) result(stat) bind(C, name="fdq_engine_build_block_fsai")
    type(c_ptr), value :: p
    real(c_double), value :: sigma
    integer(c_int), value :: level
    integer(c_int) :: stat
    type(davidson_engine), pointer :: eng
    integer :: st
    call c_f_pointer(p, eng)
    call engine_build_block_preconditioner(eng, sigma, int(level), st)
    stat = int(st, c_int)
  end function fdq_engine_build_block_fsai

  !> engine_block_preconditioner_info(eng, block_size, nnzb, longest_row, longest_col)
  subroutine fdq_engine_block_fsai_info(p, block_size, nnzb, longest_row, longest_col) bind(C, name="fdq_engine_block_fsai_info")
    type(c_ptr), value :: p
    integer(c_int), intent(out) :: block_size
    integer(c_int64_t), intent(out) :: nnzb, longest_row, longest_col
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    call engine_block_preconditioner_info(eng, block_size, nnzb, longest_row, longest_col)
  end subroutine fdq_engine_block_fsai_info

  !> engine_set_sparse(eng, which, a) with a bsr_matrix from C arrays numbered from `base` (values in Fortran order, as bsr_from_c)
  subroutine fd_engine_set_block_sparse(p, which, n, b, rp, col, vals, base, lower) bind(C, name="fd_engine_set_block_sparse")
    type(c_ptr), value :: p
    integer(c_int), value :: which, n, b, base, lower
    integer(c_int64_t), intent(in) :: rp(*)
    integer(c_int32_t), intent(in) :: col(*)
    real(c_double), intent(in) :: vals(*)
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    call engine_set_sparse(eng, int(which), bsr_from_c(n, b, rp, col, vals, base, lower))
  end subroutine fd_engine_set_block_sparse

  !> engine_set_block_sparse_device(eng, which, n, b, ...) with device arrays: returns the engine's status (0 = set; otherwise
  !> dav_last_error says why and the operator is unset) instead of stopping the process
  function fd_engine_set_block_sparse_device(p, which, n, b, rp, rp_bits, col, col_bits, vals, base, lower, row_major) result(stat) &
       bind(C, name="fd_engine_set_block_sparse_device")
    type(c_ptr), value :: p
    integer(c_int), value :: which, n, b, rp_bits, col_bits, base, lower, row_major
    type(c_ptr), value :: rp, col, vals
    integer(c_int) :: stat
    type(davidson_engine), pointer :: eng
    integer :: st
    call c_f_pointer(p, eng)
    if (iand(lower, DAV_CSR_DIAGONALS) /= 0) then          ! the engine refuses the flag by its own message (dav_last_error)
       stat = dav_set_operator_bsr_dev(eng%h, int(which - 1, c_int), b, rp, rp_bits, col, col_bits, vals, base, lower, &
            merge(DAV_BSR_ROW_MAJOR, DAV_BSR_COL_MAJOR, row_major /= 0))
       return
    end if
    call engine_set_block_sparse_device(eng, int(which), int(n), int(b), rp, col, vals, base=int(base), lower=lower /= 0, &
         row_major=row_major /= 0, row_ptr_bits=int(rp_bits), col_bits=int(col_bits), stat=st)
    stat = int(st, c_int)
  end function fd_engine_set_block_sparse_device

  !> engine_keep_value_map(eng, which, on): the next sparse set call of operator `which` keeps its value map
  subroutine fd_engine_keep_value_map(p, which, on) bind(C, name="fd_engine_keep_value_map")
    type(c_ptr), value :: p
    integer(c_int), value :: which, on
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    call engine_keep_value_map(eng, int(which), on /= 0)
  end subroutine fd_engine_keep_value_map

  !> engine_update_sparse_values(eng, which, values) with the count values of the set call (BSR: the blocks one after the other, each
  !> in the order the set door gave them - Fortran order for fd_engine_set_block_sparse)
  subroutine fd_engine_update_values(p, which, vals, count) bind(C, name="fd_engine_update_values")
    type(c_ptr), value :: p
    integer(c_int), value :: which
    integer(c_int64_t), value :: count
    real(c_double), intent(in) :: vals(count)
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    call engine_update_sparse_values(eng, int(which), vals)
  end subroutine fd_engine_update_values

  !> engine_update_sparse_values_device(eng, which, vals, stat) with a device array: returns the engine's status (0 = updated; otherwise
  !> dav_last_error says why and the operator keeps its old values) instead of stopping the process
  function fd_engine_update_values_device(p, which, vals) result(stat) bind(C, name="fd_engine_update_values_device")
    type(c_ptr), value :: p
    integer(c_int), value :: which
    type(c_ptr), value :: vals
    integer(c_int) :: stat
    type(davidson_engine), pointer :: eng
    integer :: st
    call c_f_pointer(p, eng)
    call engine_update_sparse_values_device(eng, int(which), vals, stat=st)
    stat = int(st, c_int)
  end function fd_engine_update_values_device

  !> engine_set_initial_vectors(eng, x, stat) with x(n, ncols): returns the engine's status (0 = staged; otherwise dav_last_error says
  !> why and a guess staged earlier stays staged) instead of stopping the process
  function fd_engine_set_initial_vectors(p, x, ncols) result(stat) bind(C, name="fd_engine_set_initial_vectors")
    type(c_ptr), value :: p
    integer(c_int), value :: ncols
    real(c_double), intent(in), target :: x(*)
    integer(c_int) :: stat
    type(davidson_engine), pointer :: eng
    real(c_double), pointer :: xx(:, :)
    integer :: st
    call c_f_pointer(p, eng)
    call c_f_pointer(c_loc(x), xx, [eng%n, int(ncols)])
    call engine_set_initial_vectors(eng, xx, stat=st)
    stat = int(st, c_int)
  end function fd_engine_set_initial_vectors

  !> engine_set_initial_vectors_device(eng, ptr, ldx, ncols, stat): the same from device memory, status returned
  function fd_engine_set_initial_vectors_device(p, ptr, ldx, ncols) result(stat) bind(C, name="fd_engine_set_initial_vectors_device")
    type(c_ptr), value :: p, ptr
    integer(c_int), value :: ldx, ncols
    integer(c_int) :: stat
    type(davidson_engine), pointer :: eng
    integer :: st
    call c_f_pointer(p, eng)
    call engine_set_initial_vectors_device(eng, ptr, int(ldx), int(ncols), stat=st)
    stat = int(st, c_int)
  end function fd_engine_set_initial_vectors_device

  !> engine_keep_result_as_guess(eng, on)
  subroutine fd_engine_keep_result_as_guess(p, on) bind(C, name="fd_engine_keep_result_as_guess")
    type(c_ptr), value :: p
    integer(c_int), value :: on
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    call engine_keep_result_as_guess(eng, on /= 0)
  end subroutine fd_engine_keep_result_as_guess

  !> The one-call front ends with initial_vectors= : x0(n, g) is the guess; everything else as in the doors they extend.
  subroutine fd_dense_solve_guess(n, a, has_b, b, lowest, method, max_it, tol, max_dim, g, x0, evals, evecs, iters) &
       bind(C, name="fd_dense_solve_guess")
    integer(c_int), value :: n, has_b, lowest, method, max_it, max_dim, g
    real(c_double), value :: tol
    real(c_double), intent(in) :: a(n, n), b(n, *), x0(n, g)
    real(c_double), intent(out) :: evals(lowest), evecs(n, lowest)
    integer(c_int), intent(out) :: iters
    call dense_solve(n, a, has_b, b, lowest, method, max_it, tol, max_dim, evals, evecs, iters, x0)
  end subroutine fd_dense_solve_guess

  subroutine fd_sparse_solve_guess(n, rp, col, vals, has_b, rpb, colb, valsb, base, lower, lowest, method, max_it, tol, max_dim, g, x0, &
       evals, evecs, iters) bind(C, name="fd_sparse_solve_guess")
    integer(c_int), value :: n, has_b, base, lower, lowest, method, max_it, max_dim, g
    integer(c_int64_t), intent(in) :: rp(n + 1), rpb(*)
    integer(c_int32_t), intent(in) :: col(*), colb(*)
    real(c_double), intent(in) :: vals(*), valsb(*), x0(n, g)
    real(c_double), value :: tol
    real(c_double), intent(out) :: evals(lowest), evecs(n, lowest)
    integer(c_int), intent(out) :: iters
    call sparse_solve(n, rp, col, vals, has_b, rpb, colb, valsb, base, lower, lowest, method, max_it, tol, max_dim, evals, evecs, iters, x0)
  end subroutine fd_sparse_solve_guess

  subroutine fd_bsr_solve_guess(n, b, rp, col, vals, has_b, rpb, colb, valsb, base, lower, lowest, method, max_it, tol, max_dim, g, x0, &
       evals, evecs, iters) bind(C, name="fd_bsr_solve_guess")
    integer(c_int), value :: n, b, has_b, base, lower, lowest, method, max_it, max_dim, g
    integer(c_int64_t), intent(in) :: rp(*), rpb(*)
    integer(c_int32_t), intent(in) :: col(*), colb(*)
    real(c_double), intent(in) :: vals(*), valsb(*), x0(n, g)
    real(c_double), value :: tol
    real(c_double), intent(out) :: evals(lowest), evecs(n, lowest)
    integer(c_int), intent(out) :: iters
    call bsr_solve(n, b, rp, col, vals, has_b, rpb, colb, valsb, base, lower, lowest, method, max_it, tol, max_dim, evals, evecs, iters, x0)
  end subroutine fd_bsr_solve_guess

  subroutine fd_free_solve_guess(n, fa, fb, lowest, max_it, tol, max_dim, g, x0, evals, evecs, iters) bind(C, name="fd_free_solve_guess")
    integer(c_int), value :: n, lowest, max_it, max_dim, g
    type(c_funptr), value :: fa, fb
    real(c_double), value :: tol
    real(c_double), intent(in) :: x0(n, g)
    real(c_double), intent(out) :: evals(lowest), evecs(n, lowest)
    integer(c_int), intent(out) :: iters
    call free_solve(fa, fb, n, lowest, max_it, tol, max_dim, evals, evecs, iters, x0)
  end subroutine fd_free_solve_guess

  !> kind 0: dense generated in HBM, 1: hashed matrix-free operator, 2: harness operator, 3: identity
  subroutine fd_engine_set_operator(p, which, kind, seed, sparsity, use_diag_val, diag_val) &
       bind(C, name="fd_engine_set_operator")
    type(c_ptr), value :: p
    integer(c_int), value :: which, kind, seed, use_diag_val
    real(c_double), value :: sparsity, diag_val
    type(davidson_engine), pointer :: eng
    real(dp), allocatable :: dv                 ! use_diag_val = 0: diag_val is absent
    call c_f_pointer(p, eng)
    if (use_diag_val /= 0) dv = diag_val
    select case (kind)
    case (0)
       call engine_generate_diagonal_dominant(eng, int(which), sparsity, dv, int(seed))
    case (1)
       call engine_set_hashed_operator(eng, int(which), sparsity, dv, int(seed))
    case (2)
       call engine_set_harness_operator(eng, int(which))
    case default
       call engine_set_identity(eng, int(which))
    end select
  end subroutine fd_engine_set_operator

  !> generalized_eigensolver(engine, ...) - device specific.  want_vectors = 0 leaves X in HBM.
  subroutine fd_engine_solve(p, lowest, method, max_it, tol, max_dim, evals, want_vectors, evecs, iters) &
       bind(C, name="fd_engine_solve")
    type(c_ptr), value :: p
    integer(c_int), value :: lowest, method, max_it, max_dim, want_vectors
    real(c_double), value :: tol
    real(c_double), intent(out) :: evals(lowest)
    real(c_double), intent(out), target :: evecs(*)
    integer(c_int), intent(out) :: iters
    type(davidson_engine), pointer :: eng
    real(c_double), pointer :: vec(:, :)
    integer :: it
    integer, allocatable :: md                  ! max_dim < 0: max_dim_sub is absent
    call c_f_pointer(p, eng)
    if (max_dim >= 0) md = max_dim
    vec => null()                               ! want_vectors = 0: eigenvectors is absent
    if (want_vectors /= 0) call c_f_pointer(c_loc(evecs), vec, [eng%n, int(lowest)])
    call generalized_eigensolver(eng, evals, vec, lowest, method_label(method), max_it, tol, it, md)
    iters = it
  end subroutine fd_engine_solve

  !> wall time of the last solve on this engine by phase (davidson_engine%phase_seconds)
  subroutine fd_engine_phase_seconds(p, out) bind(C, name="fd_engine_phase_seconds")
    type(c_ptr), value :: p
    real(c_double), intent(out) :: out(8)
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    out = eng%phase_seconds
  end subroutine fd_engine_phase_seconds

  !> what the dense front end decides before it uploads (davidson_device: fits_as_full_rows): 1 = nmat matrices of order n fit the
  !> engine's device as full rows, 0 = the front end switches to symmetric tiles
  function fd_engine_fits_as_full_rows(p, n, nmat) bind(C, name="fd_engine_fits_as_full_rows") result(fits)
    type(c_ptr), value :: p
    integer(c_int), value :: n, nmat
    integer(c_int) :: fits
    type(davidson_engine), pointer :: eng
    call c_f_pointer(p, eng)
    fits = merge(1_c_int, 0_c_int, fits_as_full_rows(eng, int(n), int(nmat)))
  end function fd_engine_fits_as_full_rows

  ! ---- helper modules (unit tests mirror src/tests/test_call_lapack.f90) ----------------------------
  subroutine fd_lapack_eigensolver(n, mtx, has_stx, stx, evals, evecs) bind(C, name="fd_lapack_eigensolver")
    integer(c_int), value :: n, has_stx
    real(c_double), intent(in) :: mtx(n, n)
    real(c_double), intent(in), target :: stx(n, *)
    real(c_double), intent(out) :: evals(n), evecs(n, n)
    real(c_double), pointer :: sp(:, :)
    sp => null()                                ! has_stx = 0: stx is absent
    if (has_stx /= 0) sp => stx(:, 1:n)
    call lapack_generalized_eigensolver(mtx, evals, evecs, sp)
  end subroutine fd_lapack_eigensolver

  subroutine fd_lapack_rayleigh_ritz(n, mtx, has_stx, stx, nvec, evals, evecs) bind(C, name="fd_lapack_rayleigh_ritz")
    integer(c_int), value :: n, has_stx, nvec
    real(c_double), intent(in) :: mtx(n, n)
    real(c_double), intent(in), target :: stx(n, *)
    real(c_double), intent(out) :: evals(n), evecs(n, n)
    real(c_double), pointer :: sp(:, :)
    sp => null()
    if (has_stx /= 0) sp => stx(:, 1:n)
    call lapack_rayleigh_ritz(mtx, evals, evecs, int(nvec), sp)
  end subroutine fd_lapack_rayleigh_ritz

  subroutine fd_lapack_qr(m, n, basis) bind(C, name="fd_lapack_qr")
    integer(c_int), value :: m, n
    real(c_double), intent(inout) :: basis(m, n)
    call lapack_qr(basis)
  end subroutine fd_lapack_qr

  subroutine fd_lapack_solver(n, arr, brr) bind(C, name="fd_lapack_solver")
    integer(c_int), value :: n
    real(c_double), intent(inout) :: arr(n, n), brr(n, 1)
    call lapack_solver(arr, brr)
  end subroutine fd_lapack_solver

  subroutine fd_lapack_matmul(ta, tb, m, k, n, a, b, c) bind(C, name="fd_lapack_matmul")
    integer(c_int), value :: ta, tb, m, k, n
    real(c_double), intent(in), target :: a(*), b(*)
    real(c_double), intent(out) :: c(m, n)
    real(c_double), pointer :: am(:, :), bm(:, :)
    character(len=1) :: ca, cb
    ca = merge('T', 'N', ta /= 0)
    cb = merge('T', 'N', tb /= 0)
    if (ta /= 0) then
       call c_f_pointer(c_loc(a), am, [k, m])
    else
       call c_f_pointer(c_loc(a), am, [m, k])
    end if
    if (tb /= 0) then
       call c_f_pointer(c_loc(b), bm, [n, k])
    else
       call c_f_pointer(c_loc(b), bm, [k, n])
    end if
    c = lapack_matmul(ca, cb, am, bm)
  end subroutine fd_lapack_matmul

  subroutine fd_lapack_sort(n, decreasing, vector, keys) bind(C, name="fd_lapack_sort")
    integer(c_int), value :: n, decreasing
    real(c_double), intent(inout) :: vector(n)
    integer(c_int), intent(out) :: keys(n)
    keys = lapack_sort(merge('D', 'I', decreasing /= 0), vector)
  end subroutine fd_lapack_sort

  subroutine fd_generate_preconditioner(n, diag, dim_sub, precond) bind(C, name="fd_generate_preconditioner")
    integer(c_int), value :: n, dim_sub
    real(c_double), intent(inout) :: diag(n)
    real(c_double), intent(out) :: precond(n, dim_sub)
    precond = generate_preconditioner(diag, dim_sub)
  end subroutine fd_generate_preconditioner

  subroutine fd_generate_diagonal_dominant(n, sparsity, use_diag_val, diag_val, seed, arr) &
       bind(C, name="fd_generate_diagonal_dominant")
    integer(c_int), value :: n, use_diag_val, seed
    real(c_double), value :: sparsity, diag_val
    real(c_double), intent(out) :: arr(n, n)
    real(dp) :: sp
    real(dp), allocatable :: dv                 ! use_diag_val = 0: diag_val is absent
    sp = sparsity
    if (use_diag_val /= 0) dv = diag_val
    arr = generate_diagonal_dominant(n, sp, dv, int(seed))
  end subroutine fd_generate_diagonal_dominant

  subroutine fd_norm(n, v, res) bind(C, name="fd_norm")
    integer(c_int), value :: n
    real(c_double), intent(in) :: v(n)
    real(c_double), intent(out) :: res
    res = norm(v)
  end subroutine fd_norm

end module davidson_c_api
