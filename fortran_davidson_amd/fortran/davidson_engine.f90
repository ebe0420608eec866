!> The handle of a device-resident eigenproblem and everything that sets it up: engine creation, the operators A and B (dense from
!> host memory or a file, generated, matrix-free device operators, the caller's own kernel), storage, communicator, the opt-in knobs
!> of a solve.  Thin Fortran faces of the C ABI (include/davidson_hip.h); the solve itself is module davidson_device (davidson.f90).
module davidson_engine_setup
  use, intrinsic :: iso_c_binding
  use numeric_kinds, only: dp
  use davidson_hip_c
  use davidson_knobs, only: basis_capacity
  implicit none
  private
  public :: davidson_engine, engine_create, engine_destroy, engine_set_dense, engine_set_storage, fits_as_full_rows, engine_set_device_rr, &
       engine_set_inner_precision, engine_read_matrix, engine_dense_begin, engine_dense_put_rows, engine_dense_end, &
       engine_set_correction_policy, engine_generate_diagonal_dominant, engine_set_hashed_operator, engine_set_harness_operator, &
       engine_set_identity, engine_set_device_operator, engine_comm_unique_id, engine_comm_init, davidson_free_buffers, &
       engine_set_initial_vectors, engine_set_initial_vectors_device, engine_keep_result_as_guess, engine_build_preconditioner, &
       engine_preconditioner_info, engine_build_block_preconditioner, engine_block_preconditioner_info

  !> Handle of a device-resident problem: operators A (and B) plus all work panels in HBM.
  type :: davidson_engine
     type(c_ptr) :: h = c_null_ptr
     integer :: n = 0
     integer :: max_cols = 0
     logical :: gev = .false.
     integer :: policy = 0          !< POLICY_ALL (the reference) or POLICY_UNCONVERGED (opt-in)
     !> .true. when operator A is matrix-free (a device operator instead of a stored matrix): the solve then
     !> follows the reference's matrix-free driver - convergence of all wanted pairs tested at once, no
     !> sticky flags (src/davidson.f90:416) - instead of the dense one (:176)
     logical :: free_semantics = .false.
     !> opt-in (engine_set_device_rr / DAVIDSON_DEVICE_RR=1): the Rayleigh-Ritz problem is solved on the device
     !> (one-workgroup Jacobi, order <= 128) and the projected matrices, Ritz values and vectors never leave HBM
     logical :: device_rr = .false.
     !> Wall time of the last solve on this engine by phase (seconds): 1 setup (init basis + first projection),
     !> 2 host Rayleigh-Ritz (DSYEV/DSYGV), 3 Ritz/residue/correction phase, 4 orthonormalisation,
     !> 5 operator apply (expand), 6 projection, 7 restart, 8 GJD inner solves.  Printed when the
     !> environment variable DAVIDSON_VERBOSE is set; never printed otherwise (drop-in silence).
     real(dp) :: phase_seconds(8) = 0.0_dp
  end type davidson_engine

  !> Correction policies of the outer loop (module davidson_loop: reference_policy_loop runs the first two, davidson_locking_loop the third)
  integer, parameter, public :: POLICY_ALL = 0, POLICY_UNCONVERGED = 1, POLICY_LOCKING = 2

contains

  !> Give the device and pinned blocks the library keeps from the engine destroyed last back to the device (the buffer cache of
  !> include/davidson_hip.h: a call per eigenproblem - the reference's interface - otherwise pays hipMalloc / hipFree of the whole
  !> problem every time).  What mkl_free_buffers is to MKL.
  subroutine davidson_free_buffers()
    integer(c_int) :: ierr
    ierr = dav_free_buffers()
  end subroutine davidson_free_buffers

  !> Do `nmat` dense operators of order n fit the engine's device as full rows (8 n^2 bytes each), with a tenth of the memory left
  !> for the panels and the partial-sum slabs?  (dav_device_memory: what is free now.)
  function fits_as_full_rows(eng, n, nmat) result(fits)
    type(davidson_engine), intent(in) :: eng
    integer, intent(in) :: n, nmat
    logical :: fits
    integer(c_int64_t) :: free_bytes, total_bytes
    call check_dav(dav_device_memory(eng%h, free_bytes, total_bytes), "dav_device_memory")
    fits = 8.0_dp * real(n, dp) * real(n, dp) * real(nmat, dp) <= 0.9_dp * real(free_bytes, dp)
  end function fits_as_full_rows

  subroutine engine_create(eng, n, lowest, max_dim_sub, gev, device, rank, nranks)
    type(davidson_engine), intent(out) :: eng
    integer, intent(in) :: n, lowest
    integer, intent(in), optional :: max_dim_sub, device, rank, nranks
    logical, intent(in), optional :: gev
    integer :: max_dim, dev, rk, nr, envlen, envstat
    character(len=32) :: envbuf
    max_dim = 10 * lowest
    if (present(max_dim_sub)) max_dim = max_dim_sub
    dev = 0; rk = 0; nr = 1
    if (present(device)) dev = device
    if (present(rank)) rk = rank
    if (present(nranks)) nr = nranks
    eng%n = n
    eng%gev = .false.
    if (present(gev)) eng%gev = gev
    eng%max_cols = basis_capacity(lowest, max_dim)
    if (dav_version() /= DAV_HIP_ABI_VERSION) then
       print *, "engine_create: libdavidson_hip.so reports ABI version ", dav_version(), ", these modules were built for ", &
            DAV_HIP_ABI_VERSION
       error stop
    end if
    call check_dav(dav_create(eng%h, int(dev, c_int), int(n, c_int64_t), int(eng%max_cols, c_int), &
         merge(1_c_int, 0_c_int, eng%gev), int(rk, c_int), int(nr, c_int)), "dav_create")
    ! engine knob that does not touch the reference's argument lists (reaches the dense and matrix-free
    ! front ends too): DAVIDSON_CORRECTION_POLICY=unconverged
    call get_environment_variable("DAVIDSON_CORRECTION_POLICY", envbuf, envlen, envstat)
    eng%policy = POLICY_ALL
    if (envstat == 0 .and. envlen > 0) call engine_set_correction_policy(eng, envbuf(1:envlen))
    call get_environment_variable("DAVIDSON_INNER_PRECISION", envbuf, envlen, envstat)
    if (envstat == 0 .and. envlen >= 2) then
       if (envbuf(1:2) == "32") call engine_set_inner_precision(eng, 32)
    end if
    call get_environment_variable("DAVIDSON_DEVICE_RR", envbuf, envlen, envstat)
    eng%device_rr = (envstat == 0 .and. envlen > 0 .and. envbuf(1:1) == "1")
  end subroutine engine_create

  !> Mixed-precision correction path (SURVEY 8f-4): bits = 32 lets the block sweeps inside the GJD correction solve
  !> read an fp32 copy of the stored symmetric tiles (fp64 products and sums); residuals, projections and the
  !> convergence test stay on the fp64 matrix.  bits = 64 (default) = the reference's precision throughout.
  subroutine engine_set_inner_precision(eng, bits)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: bits
    call check_dav(dav_set_inner_precision(eng%h, int(bits, c_int)), "dav_set_inner_precision")
  end subroutine engine_set_inner_precision

  !> Device-side Rayleigh-Ritz (SURVEY 8f-1) on or off for the solves of this engine.  Off (default): the projected
  !> problem is solved by host LAPACK, as the reference does (src/lapack_wrapper.f90:14-91).  On: one-workgroup Jacobi
  !> eigensolver on the device for bases up to 128 columns (wider bases fall back to the host); same Ritz pairs to
  !> rounding, same iteration counts; the H-down / Y-up transfers and one synchronisation per iteration disappear.
  subroutine engine_set_device_rr(eng, on)
    type(davidson_engine), intent(inout) :: eng
    logical, intent(in) :: on
    eng%device_rr = on
  end subroutine engine_set_device_rr

  !> Which Ritz pairs get a correction vector each iteration.  "all" (default) is the reference's policy:
  !> one correction per basis vector, the basis doubles (src/davidson.f90:195-213), sticky convergence on the
  !> dense path.  "unconverged" (opt-in; not in the reference, changes the iteration count): only those of
  !> the `lowest` wanted pairs whose residual is still above the tolerance are corrected, convergence is
  !> tested on all wanted pairs at once, and the basis grows by at most `lowest` columns per iteration -
  !> narrower panels, one 16-column pass of the symmetric sweep per iteration, and GJD inner solves only for
  !> the pairs that need them.  "locking" (opt-in; standard problems; the deflation the reference's header cites and never
  !> implements, src/davidson.f90:7-8): a wanted pair whose residual is below the tolerance is locked - its Ritz vector leaves the
  !> active basis, which is kept orthogonal to it, its value is final - and the Rayleigh-Ritz problem, the corrections and the
  !> restarts only concern the pairs still wanted (davidson_locking_loop in module davidson_loop; oracle:
  !> generalized_eigensolver_dense_locking).
  subroutine engine_set_correction_policy(eng, policy)
    type(davidson_engine), intent(inout) :: eng
    character(len=*), intent(in) :: policy
    select case (trim(policy))
    case ("all")
       eng%policy = POLICY_ALL
    case ("unconverged")
       eng%policy = POLICY_UNCONVERGED
    case ("locking")
       eng%policy = POLICY_LOCKING
    case default
       print *, "engine_set_correction_policy: policy must be 'all', 'unconverged' or 'locking', got '", trim(policy), "'"
       error stop
    end select
  end subroutine engine_set_correction_policy

  subroutine engine_destroy(eng)
    type(davidson_engine), intent(inout) :: eng
    if (c_associated(eng%h)) call check_dav(dav_destroy(eng%h), "dav_destroy")
    eng%h = c_null_ptr
  end subroutine engine_destroy

  subroutine engine_comm_unique_id(id)
    character(kind=c_char), intent(out) :: id(128)
    call check_dav(dav_comm_unique_id(id), "dav_comm_unique_id")
  end subroutine engine_comm_unique_id

  subroutine engine_comm_init(eng, id)
    type(davidson_engine), intent(inout) :: eng
    character(kind=c_char), intent(in) :: id(128)
    call check_dav(dav_comm_init(eng%h, id), "dav_comm_init")
  end subroutine engine_comm_init

  !> Storage of the dense operators set afterwards: "full" (default) or "symmetric" = only the lower
  !> block triangle is kept in HBM (N(N+1)/2 entries: N = 200000 fits one MI355X) and every
  !> off-diagonal tile is used twice per sweep.  Single GPU only.
  subroutine engine_set_storage(eng, storage)
    type(davidson_engine), intent(inout) :: eng
    character(len=*), intent(in) :: storage
    integer(c_int) :: mode
    select case (trim(storage))
    case ("full")
       mode = 0
    case ("symmetric")
       mode = 1
    case default
       print *, "engine_set_storage: storage must be 'full' or 'symmetric'"
       error stop
    end select
    call check_dav(dav_set_storage(eng%h, mode), "dav_set_storage")
  end subroutine engine_set_storage

  !> Upload a host matrix (full storage) as operator A (which=1) or B (which=2).
  subroutine engine_set_dense(eng, which, matrix)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    real(dp), dimension(:, :), intent(in) :: matrix
    if (size(matrix, 1) /= eng%n .or. size(matrix, 2) /= eng%n) then
       print *, "engine_set_dense: matrix must be ", eng%n, " x ", eng%n
       error stop
    end if
    call check_dav(dav_set_dense_host(eng%h, int(which - 1, c_int), matrix, int(size(matrix, 1), c_int64_t)), &
         "dav_set_dense_host")
    if (which == 1) eng%free_semantics = .false.
  end subroutine engine_set_dense

  !> Operator A (which=1) or B (which=2) from a file, streamed to HBM by blocks of rows - no host N x N
  !> array.  fmt = "text" (default): the format read_matrix reads and write_matrix writes in the reference's
  !> test_utils (src/tests/test_utils.f90:118-135,150-166: list-directed reals, row-major); fmt = "f64": raw
  !> float64, row-major, 8 n^2 bytes.
  subroutine engine_read_matrix(eng, which, path_file, fmt)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    character(len=*), intent(in) :: path_file
    character(len=*), intent(in), optional :: fmt
    integer(c_int) :: code
    code = 0
    if (present(fmt)) then
       select case (trim(fmt))
       case ("text")
          code = 0
       case ("f64")
          code = 1
       case default
          print *, "engine_read_matrix: fmt must be 'text' or 'f64'"
          error stop
       end select
    end if
    call check_dav(dav_set_dense_file(eng%h, int(which - 1, c_int), trim(path_file) // c_null_char, code), &
         "dav_set_dense_file")
    if (which == 1) eng%free_semantics = .false.
  end subroutine engine_read_matrix

  !> Streaming upload for hosts that produce the matrix row by row: begin, any number of put_rows (each a
  !> block of complete rows; rows(j, r) = element (row0 + r - 1, j), i.e. one matrix row per COLUMN of the
  !> Fortran array, which is the row-major order of the file format), end.
  subroutine engine_dense_begin(eng, which)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    call check_dav(dav_dense_begin(eng%h, int(which - 1, c_int)), "dav_dense_begin")
    if (which == 1) eng%free_semantics = .false.
  end subroutine engine_dense_begin

  subroutine engine_dense_put_rows(eng, which, row0, rows)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    integer, intent(in) :: row0                          !< 1-based global index of the first row
    real(dp), dimension(:, :), contiguous, intent(in) :: rows   !< (n, nrows)
    if (size(rows, 1) /= eng%n) then
       print *, "engine_dense_put_rows: rows must be (", eng%n, ", nrows)"
       error stop
    end if
    call check_dav(dav_dense_put_rows(eng%h, int(which - 1, c_int), int(row0 - 1, c_int64_t), &
         int(size(rows, 2), c_int64_t), rows, int(size(rows, 1), c_int64_t)), "dav_dense_put_rows")
  end subroutine engine_dense_put_rows

  subroutine engine_dense_end(eng, which)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    call check_dav(dav_dense_end(eng%h, int(which - 1, c_int)), "dav_dense_end")
  end subroutine engine_dense_end

  !> generate_diagonal_dominant(n, sparsity[, diag_val]) built directly in HBM (same entries as the
  !> host function of array_utils with the same seed).
  subroutine engine_generate_diagonal_dominant(eng, which, sparsity, diag_val, seed)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    real(dp), intent(in) :: sparsity
    real(dp), intent(in), optional :: diag_val
    integer, intent(in), optional :: seed
    integer(c_int64_t) :: s
    real(c_double) :: dv
    s = 1
    if (present(seed)) s = int(seed, c_int64_t)
    dv = 0.0_dp
    if (present(diag_val)) dv = diag_val
    call check_dav(dav_set_dense_generated(eng%h, int(which - 1, c_int), s, sparsity, &
         merge(1_c_int, 0_c_int, present(diag_val)), dv), "dav_set_dense_generated")
    if (which == 1) eng%free_semantics = .false.
  end subroutine engine_generate_diagonal_dominant

  !> Same matrix as engine_generate_diagonal_dominant but never stored: entries are generated on
  !> the fly inside the block matvec (matrix-free device operator).
  subroutine engine_set_hashed_operator(eng, which, sparsity, diag_val, seed)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    real(dp), intent(in) :: sparsity
    real(dp), intent(in), optional :: diag_val
    integer, intent(in), optional :: seed
    integer(c_int64_t) :: s
    real(c_double) :: dv
    s = 1
    if (present(seed)) s = int(seed, c_int64_t)
    dv = 0.0_dp
    if (present(diag_val)) dv = diag_val
    call check_dav(dav_set_operator_hashed(eng%h, int(which - 1, c_int), s, sparsity, &
         merge(1_c_int, 0_c_int, present(diag_val)), dv), "dav_set_operator_hashed")
    if (which == 1) eng%free_semantics = .true.
  end subroutine engine_set_hashed_operator

  !> The operators of the reference's matrix-free tests (src/tests/test_utils.f90:38-116) evaluated
  !> on the device: which=1 -> cos generator + i on the diagonal, which=2 -> sin generator, unit diagonal.
  subroutine engine_set_harness_operator(eng, which)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    real(dp), allocatable :: e(:)
    integer :: i
    allocate(e(eng%n))
    do i = 1, eng%n
       e(i) = exp(real(i) / real(eng%n))      ! single precision on purpose (test_utils.f90:82)
    end do
    call check_dav(dav_set_operator_harness(eng%h, int(which - 1, c_int), e), "dav_set_operator_harness")
    if (which == 1) eng%free_semantics = .true.
  end subroutine engine_set_harness_operator

  !> B = I (which = 2) - or the preconditioner M = I (which = 3).
  !> Slot 3 (DAV_OP_M of include/davidson_hip.h, which says what M must be) holds the caller's preconditioner: an approximation of
  !> (A - sigma B)^-1 that "DPR" (T = M R) and "GJD" (the preconditioner of its MINRES) apply in place of the diagonal; "BDPR", "CHEB" and
  !> "LCHEB" do not read it.  It is set through engine_set_sparse, engine_set_sparse_device, engine_set_block_sparse_device,
  !> engine_set_device_operator and this routine, refreshed through engine_keep_value_map / engine_update_sparse_values(_device), replaced
  !> by setting it again and never unset.  Every other engine_set_* / engine_read_matrix / engine_dense_* / engine_generate_* routine
  !> stops with the engine's message when it is handed which = 3.
  subroutine engine_set_identity(eng, which)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    call check_dav(dav_set_operator_identity(eng%h, int(which - 1, c_int)), "dav_set_operator_identity")
  end subroutine engine_set_identity

  !> The preconditioner M BUILT from the stored operators (include/davidson_hip_precond.h; DESIGN section 29): the factorized sparse
  !> approximate inverse G^T G of A - sigma B on the pattern of tril(A)^level, level = 1 (default), 2 or 3, into slot 3.  A is a CSR
  !> operator (engine_set_sparse), B a CSR operator or the identity, A - sigma B positive definite; one rank.  A snapshot: call it again
  !> after new values.  stat present: a refused build returns its non-zero status here (dav_last_error says why; slot 3 is then unset),
  !> otherwise the program stops with the engine's message.
  subroutine engine_build_preconditioner(eng, sigma, level, stat)
    type(davidson_engine), intent(inout) :: eng
    real(dp), intent(in) :: sigma
    integer, intent(in), optional :: level
    integer, intent(out), optional :: stat
    integer(c_int) :: ierr, lv
    lv = 1_c_int
    if (present(level)) lv = int(level, c_int)
    ierr = davp_build_fsai(eng%h, real(sigma, c_double), lv)
    if (present(stat)) then
       stat = int(ierr)
    else
       call check_dav(ierr, "davp_build_fsai")
    end if
  end subroutine engine_build_preconditioner

  !> Entries of G, its longest row and the longest row of G^T of the preconditioner engine_build_preconditioner left in slot 3 (zeros
  !> when the slot holds something else)
  subroutine engine_preconditioner_info(eng, nnz, longest_row, longest_col)
    type(davidson_engine), intent(in) :: eng
    integer(c_int64_t), intent(out) :: nnz, longest_row, longest_col
    call check_dav(davp_fsai_info(eng%h, nnz, longest_row, longest_col), "davp_fsai_info")
  end subroutine engine_preconditioner_info

  !> The preconditioner M BUILT from stored BLOCK operators (include/davidson_hip_bprecond.h; DESIGN section 30): the block factorized
  !> sparse approximate inverse G^T G of A - sigma B on the pattern of tril(A)^level over the block index arrays, level = 1 (default), 2 or
  !> 3, into slot 3.  A is a BSR operator (engine_set_sparse with a bsr_matrix; engine_set_hermitian, block size 2), B a BSR operator of
  !> the same block size or the identity, A - sigma B positive definite; one rank; a block row of G holds at most 64 scalar columns.  A
  !> snapshot: call it again after new values.  stat present: a refused build returns its non-zero status here (dav_last_error says why;
  !> slot 3 is then unset), otherwise the program stops with the engine's message.
  subroutine engine_build_block_preconditioner(eng, sigma, level, stat)
    type(davidson_engine), intent(inout) :: eng
    real(dp), intent(in) :: sigma
    integer, intent(in), optional :: level
    integer, intent(out), optional :: stat
    integer(c_int) :: ierr, lv
    lv = 1_c_int
    if (present(level)) lv = int(level, c_int)
    ierr = davq_build_block_fsai(eng%h, real(sigma, c_double), lv)
    if (present(stat)) then
       stat = int(ierr)
    else
       call check_dav(ierr, "davq_build_block_fsai")
    end if
  end subroutine engine_build_block_preconditioner

  !> Block size, blocks of G, its longest block row and the longest block row of G^T of the preconditioner
  !> engine_build_block_preconditioner left in slot 3 (zeros when the slot holds something else)
  subroutine engine_block_preconditioner_info(eng, block_size, nnzb, longest_row, longest_col)
    type(davidson_engine), intent(in) :: eng
    integer(c_int), intent(out) :: block_size
    integer(c_int64_t), intent(out) :: nnzb, longest_row, longest_col
    call check_dav(davq_block_fsai_info(eng%h, block_size, nnzb, longest_row, longest_col), "davq_block_fsai_info")
  end subroutine engine_block_preconditioner_info

  !> The caller's OWN operator as a block apply on device memory: the device counterpart of the reference's matrix-free interface
  !> (src/davidson.f90:277-337 takes a procedure on host arrays).  `fn` = c_funloc of a bind(C) function with the signature
  !> dav_device_apply_fn of include/davidson_hip.h - it enqueues Y = Op(row0 : row0 + nloc, :) X on the stream it is handed (its own
  !> HIP kernels, hipBLAS, ...) - `ctx` is passed through to it, `diag` is the operator's diagonal (n entries).
  !> which = 3: the preconditioner M (see engine_set_identity); its diagonal is not read, an array of any size will do.
  subroutine engine_set_device_operator(eng, which, fn, ctx, diag)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: which
    type(c_funptr), intent(in) :: fn
    type(c_ptr), intent(in) :: ctx
    real(dp), intent(in) :: diag(:)
    if (size(diag) /= eng%n .and. which /= 3) then
       print *, "engine_set_device_operator: diag must have n entries"
       error stop
    end if
    call check_dav(dav_set_operator_device(eng%h, int(which - 1, c_int), fn, ctx, diag), "dav_set_operator_device")
  end subroutine engine_set_device_operator

  !> Warm start: the next solve on this engine begins from the columns of x (n rows; the whole array on every rank) instead of unit
  !> vectors - the eigenvectors of the previous step of an SCF iteration, a parameter scan, a time loop.  The columns need not be
  !> orthonormal (nor B-orthonormal) or independent; of a guess wider than the start basis, 2 * lowest, the leading columns are used.
  !> One-shot: the solve consumes it.  stat present: a refused guess - more columns than the engine's basis holds, an entry that is not
  !> finite, a column that is entirely zero - returns its non-zero status here (dav_last_error says why; a guess staged earlier
  !> stays staged), otherwise the program stops.
  subroutine engine_set_initial_vectors(eng, x, stat)
    type(davidson_engine), intent(inout) :: eng
    real(dp), dimension(:, :), contiguous, intent(in) :: x
    integer, intent(out), optional :: stat
    integer(c_int) :: ierr
    if (size(x, 1) /= eng%n) then
       print *, "engine_set_initial_vectors: x must have ", eng%n, " rows"
       error stop
    end if
    ierr = dav_set_guess(eng%h, x, int(size(x, 1), c_int64_t), int(size(x, 2), c_int))
    if (present(stat)) then
       stat = int(ierr)
    else
       call check_dav(ierr, "dav_set_guess")
    end if
  end subroutine engine_set_initial_vectors

  !> The same with x(ldx, ncols) in device memory of the engine's device, complete when the call is made and free again when it
  !> returns (the engine checks the pointer before it launches anything).
  subroutine engine_set_initial_vectors_device(eng, ptr, ldx, ncols, stat)
    type(davidson_engine), intent(inout) :: eng
    type(c_ptr), intent(in) :: ptr
    integer, intent(in) :: ldx, ncols
    integer, intent(out), optional :: stat
    integer(c_int) :: ierr
    ierr = dav_set_guess_dev(eng%h, ptr, int(ldx, c_int64_t), int(ncols, c_int))
    if (present(stat)) then
       stat = int(ierr)
    else
       call check_dav(ierr, "dav_set_guess_dev")
    end if
  end subroutine engine_set_initial_vectors_device

  !> Sticky switch (default off): while it is on, every solve on this engine starts from the Ritz vectors the previous solve left in
  !> HBM - nothing is copied - as long as nothing else has written that panel since.  Setting or updating an operator keeps them.
  subroutine engine_keep_result_as_guess(eng, on)
    type(davidson_engine), intent(inout) :: eng
    logical, intent(in) :: on
    call check_dav(dav_keep_result_as_guess(eng%h, merge(1_c_int, 0_c_int, on)), "dav_keep_result_as_guess")
  end subroutine engine_keep_result_as_guess

end module davidson_engine_setup
