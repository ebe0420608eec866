!> MI355X-native block Davidson eigensolver behind the Fortran API of NLESC-JCER/Fortran_Davidson.
!>
!> Public surface (drop-in): module `davidson` with the generic `generalized_eigensolver`
!> (reference: src/davidson.f90:599-625) whose dense and matrix-free specifics keep the reference's
!> argument lists (src/davidson.f90:51-52, :277-278), plus `free_matmul` (src/davidson.f90:526).
!> A third specific takes a `davidson_engine` handle so that a matrix already resident in HBM (or a
!> built-in device operator) can be solved repeatedly without re-uploading.
!>
!> Design: the host keeps the control flow of the reference's outer loop (src/davidson.f90:138-229: module davidson_loop; this file
!> holds the front ends) and the m x m Rayleigh-Ritz problem (lapack_wrapper); everything N-long lives in HBM behind the
!> C ABI of include/davidson_hip.h.  Per iteration the device does ONE block sweep of A (the new
!> basis columns only) instead of the reference's (m+1) sweeps, residues come from the cached A*V
!> panel, and Householder QR of the whole basis is replaced by a block Gram-Schmidt of the new
!> columns (same span, hence the same Ritz values, residual norms and iteration counts).

module davidson_device
  use, intrinsic :: iso_c_binding
  use numeric_kinds, only: dp
  use davidson_hip_c
  use davidson_knobs
  use davidson_engine_setup
  use davidson_loop, only: davidson_device_loop
  implicit none
  private
  public :: POLICY_ALL, POLICY_UNCONVERGED, POLICY_LOCKING
  public :: davidson_engine, engine_create, engine_destroy, engine_set_dense, engine_set_storage, env_device, env_storage_symmetric, env_storage, symmetry_probe, fits_as_full_rows, engine_set_device_rr, engine_set_inner_precision, &
       engine_read_matrix, engine_dense_begin, engine_dense_put_rows, engine_dense_end, engine_set_correction_policy, &
       engine_generate_diagonal_dominant, engine_set_hashed_operator, engine_set_harness_operator, &
       engine_set_identity, engine_set_device_operator, engine_comm_unique_id, engine_comm_init, &
       generalized_eigensolver_device, generalized_eigensolver_device_guess, device_solve_impl, davidson_device_loop, basis_capacity, default_max_dim, tick, verbose, davidson_free_buffers, &
       engine_set_initial_vectors, engine_set_initial_vectors_device, engine_keep_result_as_guess, stage_initial_vectors, &
       engine_build_preconditioner, engine_preconditioner_info, engine_build_block_preconditioner, engine_block_preconditioner_info

contains

  !> initial_vectors= of the front ends: the leading columns of x that a start basis of 2 * lowest columns (and the engine) can hold
  subroutine stage_initial_vectors(eng, x, lowest)
    type(davidson_engine), intent(inout) :: eng
    real(dp), dimension(:, :), intent(in) :: x
    integer, intent(in) :: lowest
    integer :: g
    g = min(size(x, 2), 2 * lowest, eng%max_cols)
    if (g >= 1) call engine_set_initial_vectors(eng, x(:, 1:g))
  end subroutine stage_initial_vectors

  !> Solve with the operators already resident behind `eng` (third specific of the generic).
  !> Argument meaning as generalized_eigensolver_dense; `eigenvectors` is optional so that a
  !> benchmark can leave the Ritz vectors on the device.
  !> (the body of generalized_eigensolver_device and of its _guess twin; initial_vectors present: engine_set_initial_vectors first)
  subroutine device_solve_impl(eng, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, initial_vectors)
    type(davidson_engine), intent(inout) :: eng
    integer, intent(in) :: lowest
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    real(dp), dimension(:, :), intent(out), optional :: eigenvectors
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    integer :: max_dim
    max_dim = default_max_dim(lowest, max_dim_sub)
    if (basis_capacity(lowest, max_dim) > eng%max_cols) then
       print *, "generalized_eigensolver: engine created for a narrower basis than lowest/max_dim_sub need"
       error stop
    end if
    if (present(initial_vectors)) call stage_initial_vectors(eng, initial_vectors, lowest)
    ! stored matrix: the dense driver's sticky convergence flags (src/davidson.f90:176); matrix-free operator A:
    ! the matrix-free driver's all-at-once test (:416)
    call davidson_device_loop(eng%h, eng%n, lowest, method, max_iterations, tolerance, iters, max_dim, &
         eng%gev, .not. eng%free_semantics, eigenvalues, policy=eng%policy, device_rr=eng%device_rr, &
         phase_seconds=eng%phase_seconds)
    if (present(eigenvectors)) then
       call check_dav(dav_panel_get(eng%h, DAV_PANEL_X, 0_c_int, int(lowest, c_int), eigenvectors, &
            int(size(eigenvectors, 1), c_int64_t)), "dav_panel_get")
    end if
  end subroutine device_solve_impl

  !> The specific of the generic with the reference's argument list (device_solve_impl does the work).
  subroutine generalized_eigensolver_device(eng, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub)
    integer, intent(in) :: lowest
    type(davidson_engine), intent(inout) :: eng
    real(dp), dimension(:, :), intent(out), optional :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    call device_solve_impl(eng, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub)
  end subroutine generalized_eigensolver_device

  !> The same with initial_vectors= (keyword; not in the reference): the solve starts from these columns instead of unit vectors.
  !> A specific of its own, so that the one above keeps the reference's argument list - and its binary interface - exactly.
  subroutine generalized_eigensolver_device_guess(eng, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, initial_vectors)
    integer, intent(in) :: lowest
    type(davidson_engine), intent(inout) :: eng
    real(dp), dimension(:, :), intent(out), optional :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    real(dp), dimension(:, :), intent(in) :: initial_vectors
    call device_solve_impl(eng, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, initial_vectors)
  end subroutine generalized_eigensolver_device_guess

end module davidson_device


module davidson_dense
  use, intrinsic :: iso_c_binding
  use numeric_kinds, only: dp
  use davidson_hip_c
  use davidson_device
  implicit none
  private
  public :: generalized_eigensolver_dense, generalized_eigensolver_dense_guess

contains

  !> Dense front-end, argument list of the reference (src/davidson.f90:51-52, :74-83): the matrices
  !> are uploaded to HBM, solved there and everything is released before returning (the reference
  !> keeps no state across calls either, src/davidson.f90:238-244).
  !> (the body of the specific below and of its _guess twin, which passes initial_vectors)
  subroutine dense_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, initial_vectors)
    integer, intent(in) :: lowest
    real(dp), dimension(:, :), intent(in) :: matrix
    real(dp), dimension(:, :), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in) :: max_iterations
    integer, intent(in), optional :: max_dim_sub
    real(dp), intent(in) :: tolerance
    character(len=*), intent(in) :: method
    integer, intent(out) :: iters

    type(davidson_engine) :: eng
    integer :: max_dim
    logical :: symmetric
    real(dp) :: t(5)

    max_dim = default_max_dim(lowest, max_dim_sub)
    t(1) = tick()
    call engine_create(eng, size(matrix, 1), lowest, max_dim, present(second_matrix), env_device())
    ! Storage of the uploaded operators.  The reference ASSUMES a symmetric matrix (it never checks; its DPR / GJD and DSYEV steps
    ! are only meaningful for one), so only the lower block triangle needs to cross PCIe and stay in HBM: half the upload - which
    ! is what a drop-in call spends its time on (N=20000: 60 of 62 ms) - and half the bytes per sweep.  Default (round 5): symmetric
    ! tiles when a cheap exact probe of the host matrices finds them symmetric (symmetry_probe: whole sampled rows against their
    ! columns); a matrix that fails the probe is uploaded in full and swept as the reference's DGEMM would read it.
    ! DAVIDSON_STORAGE=full | symmetric overrides; full rows that do not fit the device fall back to symmetric tiles as before.
    select case (env_storage())
    case (1)
       symmetric = .true.
    case (0)
       symmetric = .not. fits_as_full_rows(eng, size(matrix, 1), merge(2, 1, present(second_matrix)))
    case default
       symmetric = symmetry_probe(matrix)
       if (symmetric .and. present(second_matrix)) symmetric = symmetry_probe(second_matrix)
       if (.not. symmetric) symmetric = .not. fits_as_full_rows(eng, size(matrix, 1), merge(2, 1, present(second_matrix)))
    end select
    if (symmetric) call engine_set_storage(eng, "symmetric")
    t(2) = tick()
    call engine_set_dense(eng, 1, matrix)
    if (present(second_matrix)) call engine_set_dense(eng, 2, second_matrix)
    t(3) = tick()
    call device_solve_impl(eng, eigenvalues, eigenvectors, lowest, method, max_iterations, &
         tolerance, iters, max_dim, initial_vectors)
    t(4) = tick()
    call engine_destroy(eng)
    t(5) = tick()
    if (verbose()) print "(a, i0, a, l1, a, 4f9.3)", "davidson dense call: n=", size(matrix, 1), " symmetric tiles=", symmetric, &
         " ms[create+probe upload solve+download destroy]=", (t(2:5) - t(1:4)) * 1.0e3_dp
  end subroutine dense_solve_impl

  !> The specific of the generic with the reference's argument list (dense_solve_impl does the work).
  subroutine generalized_eigensolver_dense(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix)
    integer, intent(in) :: lowest
    real(dp), dimension(:, :), intent(in) :: matrix
    real(dp), dimension(:, :), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    call dense_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix)
  end subroutine generalized_eigensolver_dense

  !> The same with initial_vectors= (keyword; not in the reference): the solve starts from these columns instead of unit vectors.
  !> A specific of its own, so that the one above keeps the reference's argument list - and its binary interface - exactly.
  subroutine generalized_eigensolver_dense_guess(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, initial_vectors)
    integer, intent(in) :: lowest
    real(dp), dimension(:, :), intent(in) :: matrix
    real(dp), dimension(:, :), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    real(dp), dimension(:, :), intent(in) :: initial_vectors
    call dense_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix, initial_vectors)
  end subroutine generalized_eigensolver_dense_guess

end module davidson_dense


module davidson_free
  use, intrinsic :: iso_c_binding
  use numeric_kinds, only: dp
  use davidson_hip_c
  use davidson_device
  implicit none
  private
  public :: generalized_eigensolver_free, generalized_eigensolver_free_guess, free_matmul

contains

  !> Matrix-free front-end, argument list of the reference (src/davidson.f90:277-278, :305-337):
  !> A and B arrive as host callbacks that map a block of vectors.  The basis, A*V, B*V and every
  !> N-long product live on the GPU; only the NEW basis columns travel to the host for the callback
  !> (the reference re-applies both operators to the whole basis each iteration, :378-379).
  !> As in the reference the problem is always generalized and the correction always DPR (:428),
  !> and convergence is tested on all pairs at once (:416).
  !> (the body of the specific below and of its _guess twin, which passes initial_vectors)
  subroutine free_solve_impl(fun_matrix_gemv, eigenvalues, ritz_vectors, lowest, method, &
       max_iterations, tolerance, iters, max_dim_sub, fun_second_matrix_gemv, initial_vectors)
    integer, intent(in) :: lowest
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    real(dp), dimension(:, :), intent(out) :: ritz_vectors
    integer, intent(in) :: max_iterations
    integer, intent(in), optional :: max_dim_sub
    real(dp), intent(in) :: tolerance
    character(len=*), intent(in) :: method
    integer, intent(out) :: iters
    interface
       function fun_matrix_gemv(input_vect) result(output_vect)
         use numeric_kinds, only: dp
         real(dp), dimension(:, :), intent(in) :: input_vect
         real(dp), dimension(size(input_vect, 1), size(input_vect, 2)) :: output_vect
       end function fun_matrix_gemv
       function fun_second_matrix_gemv(input_vect) result(output_vect)
         use numeric_kinds, only: dp
         real(dp), dimension(:, :), intent(in) :: input_vect
         real(dp), dimension(size(input_vect, 1), size(input_vect, 2)) :: output_vect
       end function fun_second_matrix_gemv
    end interface

    type(davidson_engine) :: eng
    real(dp), allocatable :: diag_a(:), diag_b(:)
    integer :: n, max_dim

    n = size(ritz_vectors, 1)
    max_dim = default_max_dim(lowest, max_dim_sub)
    allocate(diag_a(n), diag_b(n))
    call extract_diagonal_blocked(fun_matrix_gemv, n, diag_a)
    call extract_diagonal_blocked(fun_second_matrix_gemv, n, diag_b)

    call engine_create(eng, n, lowest, max_dim, .true., env_device())
    call check_dav(dav_set_operator_host(eng%h, DAV_OP_A, diag_a), "dav_set_operator_host")
    call check_dav(dav_set_operator_host(eng%h, DAV_OP_B, diag_b), "dav_set_operator_host")
    if (present(initial_vectors)) call stage_initial_vectors(eng, initial_vectors, lowest)
    call davidson_device_loop(eng%h, n, lowest, method, max_iterations, tolerance, iters, max_dim, .true., &
         .false., eigenvalues, fun_matrix_gemv, fun_second_matrix_gemv, eng%policy, eng%device_rr)
    call check_dav(dav_panel_get(eng%h, DAV_PANEL_X, 0_c_int, int(lowest, c_int), ritz_vectors, &
         int(size(ritz_vectors, 1), c_int64_t)), "dav_panel_get")
    call engine_destroy(eng)
  end subroutine free_solve_impl

  !> The specific of the generic with the reference's argument list (free_solve_impl does the work).
  subroutine generalized_eigensolver_free(fun_matrix_gemv, eigenvalues, ritz_vectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, fun_second_matrix_gemv)
    integer, intent(in) :: lowest
    real(dp), dimension(:, :), intent(out) :: ritz_vectors
    integer, intent(in), optional :: max_dim_sub
    interface
       function fun_matrix_gemv(input_vect) result(output_vect)
         use numeric_kinds, only: dp
         real(dp), dimension(:, :), intent(in) :: input_vect
         real(dp), dimension(size(input_vect, 1), size(input_vect, 2)) :: output_vect
       end function fun_matrix_gemv
       function fun_second_matrix_gemv(input_vect) result(output_vect)
         use numeric_kinds, only: dp
         real(dp), dimension(:, :), intent(in) :: input_vect
         real(dp), dimension(size(input_vect, 1), size(input_vect, 2)) :: output_vect
       end function fun_second_matrix_gemv
    end interface
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    call free_solve_impl(fun_matrix_gemv, eigenvalues, ritz_vectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, fun_second_matrix_gemv)
  end subroutine generalized_eigensolver_free

  !> The same with initial_vectors= (keyword; not in the reference): the solve starts from these columns instead of unit vectors.
  !> A specific of its own, so that the one above keeps the reference's argument list - and its binary interface - exactly.
  subroutine generalized_eigensolver_free_guess(fun_matrix_gemv, eigenvalues, ritz_vectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, fun_second_matrix_gemv, initial_vectors)
    integer, intent(in) :: lowest
    real(dp), dimension(:, :), intent(out) :: ritz_vectors
    integer, intent(in), optional :: max_dim_sub
    interface
       function fun_matrix_gemv(input_vect) result(output_vect)
         use numeric_kinds, only: dp
         real(dp), dimension(:, :), intent(in) :: input_vect
         real(dp), dimension(size(input_vect, 1), size(input_vect, 2)) :: output_vect
       end function fun_matrix_gemv
       function fun_second_matrix_gemv(input_vect) result(output_vect)
         use numeric_kinds, only: dp
         real(dp), dimension(:, :), intent(in) :: input_vect
         real(dp), dimension(size(input_vect, 1), size(input_vect, 2)) :: output_vect
       end function fun_second_matrix_gemv
    end interface
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    real(dp), dimension(:, :), intent(in) :: initial_vectors
    call free_solve_impl(fun_matrix_gemv, eigenvalues, ritz_vectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, fun_second_matrix_gemv, initial_vectors)
  end subroutine generalized_eigensolver_free_guess

  !> Diagonal of an operator known only through its block apply: same N unit-vector probes as
  !> extract_diagonal_free (src/davidson.f90:490-523), sent through the callback 64 at a time.
  subroutine extract_diagonal_blocked(fun, n, diag)
    integer, intent(in) :: n
    real(dp), intent(out) :: diag(n)
    interface
       function fun(input_vect) result(output_vect)
         use numeric_kinds, only: dp
         real(dp), dimension(:, :), intent(in) :: input_vect
         real(dp), dimension(size(input_vect, 1), size(input_vect, 2)) :: output_vect
       end function fun
    end interface
    integer, parameter :: chunk = 64
    real(dp), allocatable :: probe(:, :), image(:, :)
    integer :: i0, k, j
    do i0 = 1, n, chunk
       k = min(chunk, n - i0 + 1)
       allocate(probe(n, k), image(n, k))
       probe = 0.0_dp
       do j = 1, k
          probe(i0 + j - 1, j) = 1.0_dp
       end do
       image = fun(probe)
       do j = 1, k
          diag(i0 + j - 1) = image(i0 + j - 1, j)
       end do
       deallocate(probe, image)
    end do
  end subroutine extract_diagonal_blocked

  !> Apply a matrix given by a row generator fun(i, dim) to a block (public helper of the reference,
  !> src/davidson.f90:526-569).  Host code: it serves user callbacks; rows are independent.
  function free_matmul(fun, array) result(matrix)
    real(dp), dimension(:, :), intent(in) :: array
    real(dp), dimension(size(array, 1), size(array, 2)) :: matrix
    interface
       function fun(i, dim) result(vec)
         use numeric_kinds, only: dp
         integer, intent(in) :: i
         integer, intent(in) :: dim
         real(dp), dimension(dim) :: vec
       end function fun
    end interface
    real(dp), allocatable :: row(:)
    integer :: i, n
    n = size(array, 1)
    !$OMP PARALLEL DO PRIVATE(i, row)
    do i = 1, n
       row = fun(i, n)
       matrix(i, :) = matmul(row, array)
    end do
    !$OMP END PARALLEL DO
  end function free_matmul

end module davidson_free


module davidson_csr
  use, intrinsic :: iso_c_binding
  use numeric_kinds, only: dp
  use davidson_device
  use davidson_sparse
  implicit none
  private
  public :: generalized_eigensolver_sparse, generalized_eigensolver_bsr, generalized_eigensolver_sparse_guess, generalized_eigensolver_bsr_guess
  public :: generalized_eigensolver_sparse_precond_csr, generalized_eigensolver_sparse_precond_bsr, generalized_eigensolver_bsr_precond_csr, &
       generalized_eigensolver_bsr_precond_bsr
  public :: generalized_eigensolver_coo, generalized_eigensolver_coo_precond_coo, generalized_eigensolver_coo_precond_csr, &
       generalized_eigensolver_coo_precond_bsr

contains

  !> Sparse front-end: the argument list of generalized_eigensolver_dense with csr_matrix operators (module davidson_sparse).  The
  !> matrices go to HBM as CSR rows, are solved there with the engine's CSR kernel and are released before returning.
  subroutine sparse_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, initial_vectors, precond_csr, precond_bsr)
    integer, intent(in) :: lowest
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    type(csr_matrix), intent(in) :: matrix
    type(csr_matrix), intent(in), optional :: second_matrix
    type(csr_matrix), intent(in), optional :: precond_csr      !< preconditioner= of the front ends: slot 3 of the engine
    type(bsr_matrix), intent(in), optional :: precond_bsr
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in) :: max_iterations
    integer, intent(in), optional :: max_dim_sub
    real(dp), intent(in) :: tolerance
    character(len=*), intent(in) :: method
    integer, intent(out) :: iters

    type(davidson_engine) :: eng
    integer :: max_dim

    max_dim = default_max_dim(lowest, max_dim_sub)
    call engine_create(eng, matrix%n, lowest, max_dim, present(second_matrix), env_device())
    call engine_set_sparse(eng, 1, matrix)
    if (present(second_matrix)) call engine_set_sparse(eng, 2, second_matrix)
    if (present(precond_csr)) call engine_set_sparse(eng, 3, precond_csr)
    if (present(precond_bsr)) call engine_set_sparse(eng, 3, precond_bsr)
    call device_solve_impl(eng, eigenvalues, eigenvectors, lowest, method, max_iterations, &
         tolerance, iters, max_dim, initial_vectors)
    call engine_destroy(eng)
  end subroutine sparse_solve_impl

  !> The specific of the generic with the reference's argument list (sparse_solve_impl does the work).
  subroutine generalized_eigensolver_sparse(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix)
    integer, intent(in) :: lowest
    type(csr_matrix), intent(in) :: matrix
    type(csr_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    call sparse_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix)
  end subroutine generalized_eigensolver_sparse

  !> The same with initial_vectors= (keyword; not in the reference): the solve starts from these columns instead of unit vectors.
  !> A specific of its own, so that the one above keeps the reference's argument list - and its binary interface - exactly.
  subroutine generalized_eigensolver_sparse_guess(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, initial_vectors)
    integer, intent(in) :: lowest
    type(csr_matrix), intent(in) :: matrix
    type(csr_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    real(dp), dimension(:, :), intent(in) :: initial_vectors
    call sparse_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix, initial_vectors)
  end subroutine generalized_eigensolver_sparse_guess

  !> Block-sparse front-end: the same argument list with bsr_matrix operators (module davidson_sparse).  The matrices go to HBM as
  !> blocks, are solved there with the engine's matrix-core BSR kernel and are released before returning.
  subroutine bsr_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, initial_vectors, precond_csr, precond_bsr)
    integer, intent(in) :: lowest
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    type(bsr_matrix), intent(in) :: matrix
    type(bsr_matrix), intent(in), optional :: second_matrix
    type(csr_matrix), intent(in), optional :: precond_csr      !< preconditioner= of the front ends: slot 3 of the engine
    type(bsr_matrix), intent(in), optional :: precond_bsr
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in) :: max_iterations
    integer, intent(in), optional :: max_dim_sub
    real(dp), intent(in) :: tolerance
    character(len=*), intent(in) :: method
    integer, intent(out) :: iters

    type(davidson_engine) :: eng
    integer :: max_dim

    max_dim = default_max_dim(lowest, max_dim_sub)
    call engine_create(eng, matrix%n, lowest, max_dim, present(second_matrix), env_device())
    call engine_set_sparse(eng, 1, matrix)
    if (present(second_matrix)) call engine_set_sparse(eng, 2, second_matrix)
    if (present(precond_csr)) call engine_set_sparse(eng, 3, precond_csr)
    if (present(precond_bsr)) call engine_set_sparse(eng, 3, precond_bsr)
    call device_solve_impl(eng, eigenvalues, eigenvectors, lowest, method, max_iterations, &
         tolerance, iters, max_dim, initial_vectors)
    call engine_destroy(eng)
  end subroutine bsr_solve_impl

  !> The specific of the generic with the reference's argument list (bsr_solve_impl does the work).
  subroutine generalized_eigensolver_bsr(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix)
    integer, intent(in) :: lowest
    type(bsr_matrix), intent(in) :: matrix
    type(bsr_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    call bsr_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix)
  end subroutine generalized_eigensolver_bsr

  !> The same with initial_vectors= (keyword; not in the reference): the solve starts from these columns instead of unit vectors.
  !> A specific of its own, so that the one above keeps the reference's argument list - and its binary interface - exactly.
  subroutine generalized_eigensolver_bsr_guess(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, initial_vectors)
    integer, intent(in) :: lowest
    type(bsr_matrix), intent(in) :: matrix
    type(bsr_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    real(dp), dimension(:, :), intent(in) :: initial_vectors
    call bsr_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix, initial_vectors)
  end subroutine generalized_eigensolver_bsr_guess

  !> The same with preconditioner= (keyword; not in the reference), a csr_matrix: the caller's approximation of (A - sigma B)^-1, which
  !> "DPR" and "GJD" apply in place of the diagonal (slot 3 of the engine: engine_set_identity says what it must be).  initial_vectors=
  !> may accompany it.  A specific of its own, as for initial_vectors=.
  subroutine generalized_eigensolver_sparse_precond_csr(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, preconditioner, initial_vectors)
    integer, intent(in) :: lowest
    type(csr_matrix), intent(in) :: matrix
    type(csr_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    type(csr_matrix), intent(in) :: preconditioner
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    call sparse_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix, initial_vectors, precond_csr=preconditioner)
  end subroutine generalized_eigensolver_sparse_precond_csr

  !> The same with preconditioner= (keyword; not in the reference), a bsr_matrix: the caller's approximation of (A - sigma B)^-1, which
  !> "DPR" and "GJD" apply in place of the diagonal (slot 3 of the engine: engine_set_identity says what it must be).  initial_vectors=
  !> may accompany it.  A specific of its own, as for initial_vectors=.
  subroutine generalized_eigensolver_sparse_precond_bsr(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, preconditioner, initial_vectors)
    integer, intent(in) :: lowest
    type(csr_matrix), intent(in) :: matrix
    type(csr_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    type(bsr_matrix), intent(in) :: preconditioner
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    call sparse_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix, initial_vectors, precond_bsr=preconditioner)
  end subroutine generalized_eigensolver_sparse_precond_bsr

  !> The same with preconditioner= (keyword; not in the reference), a csr_matrix: the caller's approximation of (A - sigma B)^-1, which
  !> "DPR" and "GJD" apply in place of the diagonal (slot 3 of the engine: engine_set_identity says what it must be).  initial_vectors=
  !> may accompany it.  A specific of its own, as for initial_vectors=.
  subroutine generalized_eigensolver_bsr_precond_csr(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, preconditioner, initial_vectors)
    integer, intent(in) :: lowest
    type(bsr_matrix), intent(in) :: matrix
    type(bsr_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    type(csr_matrix), intent(in) :: preconditioner
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    call bsr_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix, initial_vectors, precond_csr=preconditioner)
  end subroutine generalized_eigensolver_bsr_precond_csr

  !> The same with preconditioner= (keyword; not in the reference), a bsr_matrix: the caller's approximation of (A - sigma B)^-1, which
  !> "DPR" and "GJD" apply in place of the diagonal (slot 3 of the engine: engine_set_identity says what it must be).  initial_vectors=
  !> may accompany it.  A specific of its own, as for initial_vectors=.
  subroutine generalized_eigensolver_bsr_precond_bsr(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, preconditioner, initial_vectors)
    integer, intent(in) :: lowest
    type(bsr_matrix), intent(in) :: matrix
    type(bsr_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    type(bsr_matrix), intent(in) :: preconditioner
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    call bsr_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix, initial_vectors, precond_bsr=preconditioner)
  end subroutine generalized_eigensolver_bsr_precond_bsr

  !> COO front-end: the argument list of the sparse specific with coo_matrix operators (module davidson_sparse) - unordered triples,
  !> duplicates kept as separate terms.  The operators built are those of the csr_matrix a stable sort by row gives, bit for bit.
  subroutine coo_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, initial_vectors, precond_coo, precond_csr, precond_bsr)
    integer, intent(in) :: lowest
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    type(coo_matrix), intent(in) :: matrix
    type(coo_matrix), intent(in), optional :: second_matrix
    type(coo_matrix), intent(in), optional :: precond_coo      !< preconditioner= of the front ends: slot 3 of the engine
    type(csr_matrix), intent(in), optional :: precond_csr
    type(bsr_matrix), intent(in), optional :: precond_bsr
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in) :: max_iterations
    integer, intent(in), optional :: max_dim_sub
    real(dp), intent(in) :: tolerance
    character(len=*), intent(in) :: method
    integer, intent(out) :: iters

    type(davidson_engine) :: eng
    integer :: max_dim

    max_dim = default_max_dim(lowest, max_dim_sub)
    call engine_create(eng, matrix%n, lowest, max_dim, present(second_matrix), env_device())
    call engine_set_sparse(eng, 1, matrix)
    if (present(second_matrix)) call engine_set_sparse(eng, 2, second_matrix)
    if (present(precond_coo)) call engine_set_sparse(eng, 3, precond_coo)
    if (present(precond_csr)) call engine_set_sparse(eng, 3, precond_csr)
    if (present(precond_bsr)) call engine_set_sparse(eng, 3, precond_bsr)
    call device_solve_impl(eng, eigenvalues, eigenvectors, lowest, method, max_iterations, &
         tolerance, iters, max_dim, initial_vectors)
    call engine_destroy(eng)
  end subroutine coo_solve_impl

  !> The specific of the generic for a coo_matrix, with initial_vectors= (keyword)
  subroutine generalized_eigensolver_coo(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, initial_vectors)
    integer, intent(in) :: lowest
    type(coo_matrix), intent(in) :: matrix
    type(coo_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    call coo_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix, initial_vectors)
  end subroutine generalized_eigensolver_coo

  !> The same with preconditioner=, a coo_matrix (slot 3 of the engine); initial_vectors= may accompany it.
  subroutine generalized_eigensolver_coo_precond_coo(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, preconditioner, initial_vectors)
    integer, intent(in) :: lowest
    type(coo_matrix), intent(in) :: matrix
    type(coo_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    type(coo_matrix), intent(in) :: preconditioner
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    call coo_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix, initial_vectors, precond_coo=preconditioner)
  end subroutine generalized_eigensolver_coo_precond_coo

  !> The same with preconditioner=, a csr_matrix (slot 3 of the engine); initial_vectors= may accompany it.
  subroutine generalized_eigensolver_coo_precond_csr(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, preconditioner, initial_vectors)
    integer, intent(in) :: lowest
    type(coo_matrix), intent(in) :: matrix
    type(coo_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    type(csr_matrix), intent(in) :: preconditioner
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    call coo_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix, initial_vectors, precond_csr=preconditioner)
  end subroutine generalized_eigensolver_coo_precond_csr

  !> The same with preconditioner=, a bsr_matrix (slot 3 of the engine); initial_vectors= may accompany it.
  subroutine generalized_eigensolver_coo_precond_bsr(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix, preconditioner, initial_vectors)
    integer, intent(in) :: lowest
    type(coo_matrix), intent(in) :: matrix
    type(coo_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(:, :), intent(out) :: eigenvectors
    integer, intent(in), optional :: max_dim_sub
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    type(bsr_matrix), intent(in) :: preconditioner
    real(dp), dimension(:, :), intent(in), optional :: initial_vectors
    call coo_solve_impl(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, tolerance, iters, &
         max_dim_sub, second_matrix, initial_vectors, precond_bsr=preconditioner)
  end subroutine generalized_eigensolver_coo_precond_bsr

end module davidson_csr


module davidson_zcsr
  use numeric_kinds, only: dp
  use davidson_device
  use davidson_hermitian
  implicit none
  private
  public :: generalized_eigensolver_hermitian

contains

  !> Hermitian front-end: the argument list of the sparse specific with zcsr_matrix operators (module davidson_hermitian) and complex
  !> eigenvectors (n, lowest).  The engine is created with the real order 2 n and solves for 2 * lowest real pairs - every eigenvalue of
  !> the real form is double - from which hermitian_eigenpairs takes the complex ones.  max_dim_sub counts real columns (default: that
  !> of 2 * lowest pairs); iters is the count of the real loop.
  subroutine generalized_eigensolver_hermitian(matrix, eigenvalues, eigenvectors, lowest, method, max_iterations, &
       tolerance, iters, max_dim_sub, second_matrix)
    integer, intent(in) :: lowest
    type(zcsr_matrix), intent(in) :: matrix
    type(zcsr_matrix), intent(in), optional :: second_matrix
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    complex(dp), dimension(:, :), intent(out) :: eigenvectors
    character(len=*), intent(in) :: method
    integer, intent(in) :: max_iterations
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    integer, intent(in), optional :: max_dim_sub

    type(davidson_engine) :: eng
    real(dp), allocatable :: theta(:), v(:, :)
    integer :: max_dim

    max_dim = default_max_dim(2 * lowest, max_dim_sub)
    allocate(theta(2 * lowest), v(2 * matrix%n, 2 * lowest))
    call engine_create(eng, 2 * matrix%n, 2 * lowest, max_dim, present(second_matrix), env_device())
    call engine_set_hermitian(eng, 1, matrix)
    if (present(second_matrix)) call engine_set_hermitian(eng, 2, second_matrix)
    call device_solve_impl(eng, theta, v, 2 * lowest, method, max_iterations, tolerance, iters, max_dim)
    call engine_destroy(eng)
    call hermitian_eigenpairs(theta, v, lowest, eigenvalues, eigenvectors, second_matrix)
  end subroutine generalized_eigensolver_hermitian

end module davidson_zcsr


module davidson
  use numeric_kinds, only: dp
  use davidson_dense, only: generalized_eigensolver_dense, generalized_eigensolver_dense_guess
  use davidson_free, only: generalized_eigensolver_free, generalized_eigensolver_free_guess
  use davidson_device, only: generalized_eigensolver_device, generalized_eigensolver_device_guess, davidson_free_buffers, engine_set_initial_vectors, &
       engine_set_initial_vectors_device, engine_keep_result_as_guess
  use davidson_sparse, only: csr_matrix, bsr_matrix, coo_matrix
  use davidson_hermitian, only: zcsr_matrix
  use davidson_zcsr, only: generalized_eigensolver_hermitian
  use davidson_csr, only: generalized_eigensolver_coo, generalized_eigensolver_coo_precond_coo, generalized_eigensolver_coo_precond_csr, &
       generalized_eigensolver_coo_precond_bsr
  use davidson_csr, only: generalized_eigensolver_sparse, generalized_eigensolver_bsr, generalized_eigensolver_sparse_guess, &
       generalized_eigensolver_bsr_guess, generalized_eigensolver_sparse_precond_csr, generalized_eigensolver_sparse_precond_bsr, &
       generalized_eigensolver_bsr_precond_csr, generalized_eigensolver_bsr_precond_bsr
  implicit none
  private
  public :: generalized_eigensolver, davidson_free_buffers, csr_matrix, bsr_matrix, coo_matrix, zcsr_matrix, engine_set_initial_vectors, &
       engine_set_initial_vectors_device, engine_keep_result_as_guess

  !> Generic of the reference (src/davidson.f90:601-625), resolved by the first argument: a matrix,
  !> a block-apply procedure, (new) a device-resident `davidson_engine`, or (new) a sparse `csr_matrix` / `bsr_matrix` / `coo_matrix`, or a complex Hermitian
  !> `zcsr_matrix` (complex eigenvectors).
  interface generalized_eigensolver
     procedure generalized_eigensolver_dense
     procedure generalized_eigensolver_free
     procedure generalized_eigensolver_device
     procedure generalized_eigensolver_sparse
     procedure generalized_eigensolver_bsr
     procedure generalized_eigensolver_dense_guess
     procedure generalized_eigensolver_free_guess
     procedure generalized_eigensolver_device_guess
     procedure generalized_eigensolver_sparse_guess
     procedure generalized_eigensolver_bsr_guess
     procedure generalized_eigensolver_sparse_precond_csr
     procedure generalized_eigensolver_sparse_precond_bsr
     procedure generalized_eigensolver_bsr_precond_csr
     procedure generalized_eigensolver_coo
     procedure generalized_eigensolver_coo_precond_coo
     procedure generalized_eigensolver_coo_precond_csr
     procedure generalized_eigensolver_coo_precond_bsr
     procedure generalized_eigensolver_bsr_precond_bsr
     procedure generalized_eigensolver_hermitian
  end interface generalized_eigensolver

end module davidson
