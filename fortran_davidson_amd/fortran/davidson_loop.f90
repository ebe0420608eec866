!> The outer loop of a solve (control flow of the reference, src/davidson.f90:138-229 / :375-441) as named steps on one state.
!> davidson_device_loop sets a solve_state up, starts the basis and hands it to reference_policy_loop (policies "all", "unconverged") or to
!> davidson_locking_loop (policy "locking").  Both read as the reference's numbered steps and call the step procedures below; what only depends on
!> integers (does the basis grow, by how many columns, what a contraction keeps) is a pure procedure without engine calls.  DESIGN.md, section 26.
module davidson_loop
  use, intrinsic :: iso_c_binding
  use numeric_kinds, only: dp
  use davidson_hip_c
  use davidson_method
  use lapack_wrapper, only: lapack_rayleigh_ritz, lapack_matmul
  use array_utils, only: eye
  use davidson_knobs
  use davidson_ortho
  use davidson_engine_setup, only: POLICY_ALL, POLICY_UNCONVERGED, POLICY_LOCKING
  implicit none
  private
  public :: davidson_device_loop

  !> The N-long side of the block orthonormalisation (davidson_ortho: ortho_backend) on the engine's panels: K2 Gram launches, K3
  !> block updates, replacement columns written into the basis panel
  type, extends(ortho_backend) :: device_ortho
     type(c_ptr) :: h = c_null_ptr
     integer :: n = 0
   contains
     procedure :: gram => device_ortho_gram
     procedure :: apply => device_ortho_apply
     procedure :: unit_column => device_ortho_unit_column
     procedure :: put_column => device_ortho_put_column
  end type device_ortho

  !> Everything one solve carries from step to step (the host callbacks stay dummy procedures, handed to the steps that sweep)
  type :: solve_state
     type(c_ptr) :: h = c_null_ptr
     integer :: n, lowest, max_dim, cap, m          !< m: basis width (locking: locked or guard columns first, then the active basis)
     integer :: meth, pol                           !< DAV_METHOD_* of the correction, POLICY_*
     logical :: gev, host_ops, lazy_x, drr = .false.   !< generalized; host callbacks; Ritz vectors made at the end; Rayleigh-Ritz on the device
     logical :: sticky                              !< sticky convergence flags (src/davidson.f90:176) instead of the all-at-once test (:416)
     real(dp) :: tolerance, tol_unwanted, adaptive_c   !< of the solve; the environment knobs of the GJD inner solves: read once, in begin_solve
     integer :: refresh_every, nrestart = 0         !< every refresh_every-th restart re-applies the operators; restarts so far
     real(dp), allocatable :: hm(:, :), sm(:, :)    !< the projected matrices (cap x cap, leading dimension ld) of a host Rayleigh-Ritz
     integer(c_int64_t) :: ld
     type(device_ortho) :: dev
     real(dp) :: phase_s(8) = 0.0_dp, t0            !< wall time by phase (davidson_engine%phase_seconds) and the last lap's clock
  end type solve_state

  !> Gram blocks V^T T and T^T T of the first orthonormalisation pass, when the Ritz phase brought them back with the residual norms
  type :: gram_prefetch
     logical :: have = .false.
     real(dp), allocatable :: c(:, :), g(:, :)
  end type gram_prefetch

  abstract interface
     function block_operator(input_vect) result(output_vect)
       import :: dp
       real(dp), dimension(:, :), intent(in) :: input_vect
       real(dp), dimension(size(input_vect, 1), size(input_vect, 2)) :: output_vect
     end function block_operator
  end interface

contains

  !> The outer loop (control flow of src/davidson.f90:138-229 / :375-441) on a prepared engine.
  !> sticky = .true. reproduces the dense path's sticky convergence flags (:176), .false. the
  !> matrix-free path's all-at-once test (:416).  fun_a/fun_b present = operators applied by the
  !> host through callbacks (API-faithful matrix-free path).
  subroutine davidson_device_loop(h, n, lowest, method, max_iterations, tolerance, iters, max_dim, gev, &
       sticky, eigenvalues, fun_a, fun_b, policy, device_rr, phase_seconds)
    type(c_ptr), intent(in) :: h
    integer, intent(in) :: n, lowest, max_iterations, max_dim
    character(len=*), intent(in) :: method
    real(dp), intent(in) :: tolerance
    integer, intent(out) :: iters
    logical, intent(in) :: gev, sticky
    real(dp), dimension(lowest), intent(out) :: eigenvalues
    procedure(block_operator), optional :: fun_a, fun_b
    !> POLICY_ALL (default) = the reference: one correction per basis vector, the basis doubles.
    !> POLICY_UNCONVERGED (opt-in, changes iters): corrections only for those of the `lowest` wanted pairs
    !> whose residual is still above the tolerance; all-at-once convergence test.
    integer, intent(in), optional :: policy
    !> Rayleigh-Ritz on the device (engine_set_device_rr); bases wider than 128 columns use the host
    logical, intent(in), optional :: device_rr
    !> wall time of this solve by phase (see davidson_engine%phase_seconds)
    real(dp), intent(out), optional :: phase_seconds(8)
    type(solve_state) :: s
    integer(c_int) :: nstaged
    logical :: done
    call begin_solve()
    ! Several ranks: everything the loop decides follows from these inputs and from all-reduced (hence bitwise identical) numbers.
    ! The inputs are verified in a collective whose size does not depend on them (round-5 advisor: the per-iteration words of
    ! dav_agree_next ride on all-reduces whose element count they determine - ranks that differ in `lowest` or `max_dim` would enter
    ! those with different counts) whenever they differ from what the engine verified last: the first solve always, repeated solves
    ! with the same inputs never (dav_agree_inputs); a single rank: a no-op
    ! (the staged guess columns are an input like the others: a rank that differs stops with the message instead of hanging its peers)
    call check_dav(dav_guess_columns(h, nstaged), "dav_guess_columns")
    call check_dav(dav_agree_inputs(h, [real(n, dp), real(lowest, dp), real(max_dim, dp), real(max_iterations, dp), tolerance, &
         real(s%pol, dp), real(s%meth, dp), merge(1.0_dp, 0.0_dp, sticky), merge(1.0_dp, 0.0_dp, gev), real(nstaged, dp)], 10_c_int), &
         "dav_agree_inputs")
    s%t0 = tick()
    call start_basis(s, nstaged > 0, fun_a, fun_b)
    call lap(s, 1)

    iters = max_iterations + 1
    done = .false.
    if (s%pol == POLICY_LOCKING) then
       if (s%host_ops .or. s%drr) then
          print *, "generalized_eigensolver: the 'locking' policy serves device operators with the Rayleigh-Ritz problem on the host"
          error stop
       end if
       call davidson_locking_loop(s, max_iterations, eigenvalues, iters, done)
    else
       call reference_policy_loop(s, max_iterations, eigenvalues, iters, done, fun_a, fun_b)
    end if

    if (.not. done) then
       iters = max_iterations + 1
       print *, "Warning: Algorithm did not converge!!"
    end if
    if (verbose()) print "(a, i0, a, i0, a, 8f9.3)", "davidson: n=", n, " iters=", iters, &
         " ms[setup rr ritz ortho apply project restart gjd]=", s%phase_s * 1.0e3_dp
    if (present(phase_seconds)) phase_seconds = s%phase_s
    call check_dav(dav_set_lazy_ritz_vectors(h, 0_c_int), "dav_set_lazy_ritz_vectors")
    ! X columns 1..lowest now hold the Ritz vectors this solve returns: what the next solve starts from when the caller asked for that
    ! (dav_keep_result_as_guess).  (A locking solve that ran out of iterations may not have assembled them.)
    if (done .or. s%pol /= POLICY_LOCKING) call check_dav(dav_mark_result_as_guess(h, int(lowest, c_int)), "dav_mark_result_as_guess")

  contains

    !> The state of the solve from its inputs (the declarations of src/davidson.f90:85-122) and the engine's two per-solve switches
    subroutine begin_solve()
      s%h = h
      s%n = n
      s%lowest = lowest
      s%max_dim = max_dim
      s%tolerance = tolerance
      s%gev = gev
      s%host_ops = present(fun_a)
      s%dev%h = h
      s%dev%n = n
      s%meth = DAV_METHOD_DPR        ! host callbacks: the matrix-free driver never looks at `method`, always DPR (src/davidson.f90:428)
      if (.not. s%host_ops) s%meth = method_code(trim(method))
      if (s%meth < 0) then
         ! the reference leaves the correction undefined here (src/davidson.f90:656-669)
         print *, unknown_method_message(trim(method))
         error stop
      end if
      s%pol = POLICY_ALL
      if (present(policy)) s%pol = policy
      s%sticky = sticky .and. s%pol == POLICY_ALL
      s%m = 2 * lowest
      s%cap = basis_capacity(lowest, max_dim)
      s%ld = int(s%cap, c_int64_t)
      allocate(s%hm(s%cap, s%cap), s%sm(s%cap, s%cap))
      s%hm = 0.0_dp
      s%sm = 0.0_dp
      s%refresh_every = restart_refresh_interval()
      s%tol_unwanted = gjd_tol_unwanted()
      s%adaptive_c = gjd_adaptive_factor()
      if (present(device_rr)) s%drr = device_rr .and. s%cap <= 128
      call check_dav(dav_rr_enable(h, merge(1_c_int, 0_c_int, s%drr)), "dav_rr_enable")
      ! The Ritz vectors are what the caller gets back at the end (src/davidson.f90:186-187); the DPR correction never reads them:
      ! they are made once, when the loop stops (finish_ritz_vectors), not in every iteration.  GJD needs x_k for its correction
      ! solves and the device-side Rayleigh-Ritz keeps Y on the device: both compute X in the Ritz phase as before.
      s%lazy_x = (.not. s%drr) .and. s%meth /= DAV_METHOD_GJD
      call check_dav(dav_set_lazy_ritz_vectors(h, merge(1_c_int, 0_c_int, s%lazy_x)), "dav_set_lazy_ritz_vectors")
    end subroutine begin_solve
  end subroutine davidson_device_loop

  !> Policies "all" (the reference) and "unconverged": steps 3-7 of src/davidson.f90:138-229 on the state start_basis left.
  subroutine reference_policy_loop(s, max_iterations, eigenvalues, iters, done, fun_a, fun_b)
    type(solve_state), intent(inout) :: s
    integer, intent(in) :: max_iterations
    real(dp), intent(out) :: eigenvalues(s%lowest)
    integer, intent(inout) :: iters
    logical, intent(inout) :: done
    procedure(block_operator), optional :: fun_a, fun_b
    integer :: i, kt, ncorr, nvec
    logical :: expand_now, have_all_pairs, has_converged(s%lowest)
    real(dp) :: errors(s%lowest)
    real(dp), allocatable :: theta(:), y(:, :)
    type(gram_prefetch), target :: pre
    has_converged = .false.
    outer_loop: do i = 1, max_iterations
       ! 3. Rayleigh-Ritz on the host (the only LAPACK call on the path)
       if (allocated(theta)) deallocate(theta, y)
       allocate(theta(s%m), y(s%m, s%m))
       call growth_rule(s%pol, s%m, s%lowest, s%max_dim, s%cap, expand_now, ncorr)
       ! several ranks: the decisions of this iteration must be the same everywhere.  They are functions of these words and of
       ! the all-reduced (bitwise identical) residual norms; the words ride on the all-reduce of the Ritz phase below (no
       ! collective of their own), and a rank that differs stops with a message instead of hanging its peers
       call check_dav(dav_agree_next(s%h, [real(i, dp), real(s%m, dp), merge(1.0_dp, 0.0_dp, expand_now), real(ncorr, dp), &
            s%tolerance, real(count(has_converged), dp), real(s%pol, dp), real(s%meth, dp)], 8_c_int), "dav_agree_next")
       call probe_wanted_pairs(s, i, expand_now, theta, y, errors, has_converged, have_all_pairs, done)
       if (done) then
          eigenvalues = theta(1:s%lowest)
          iters = i
          call finish_ritz_vectors(s, y)
          exit outer_loop
       end if
       nvec = merge(s%m, min(s%m, 2 * s%lowest), s%pol == POLICY_ALL .and. expand_now)
       if (.not. s%drr .and. .not. have_all_pairs) call solve_projected(s, 1, nvec, theta, y)
       call lap(s, 2)
       ! 4. Ritz vectors, residues, their norms and the correction - one fused device phase (an iteration that ends in a restart: no correction)
       call ritz_phase(s, ncorr, s%lowest, merge(s%meth, DAV_METHOD_NONE, expand_now), theta, y, errors, pre)
       eigenvalues = theta(1:s%lowest)
       if (trace_iterations()) print "(a, i0, a, i0, a, es10.3, a, es10.3, a, i0)", "davidson trace: iteration ", i, " m=", s%m, &
            " max residual ", maxval(errors(1:s%lowest)), " min ", minval(errors(1:s%lowest)), " below tolerance ", &
            count(errors(1:s%lowest) < s%tolerance)
       call test_convergence(s, errors, has_converged, done)
       if (done .or. i == max_iterations) call finish_ritz_vectors(s, y)     ! the last Ritz pairs are what a non-converged solve returns
       if (done) then
          iters = i
          exit outer_loop
       end if
       if (expand_now) then
          ! 5. correction block T -> 6./7. orthonormalised against V and itself -> new basis columns, swept and projected
          kt = correction_count(s%pol, s%m, s%n, s%cap, count(errors >= s%tolerance))
          if (kt <= 0) then                              ! V already spans everything (policy all: unreachable, exact Ritz pairs converge)
             call finish_ritz_vectors(s, y)
             exit outer_loop
          end if
          if (s%pol /= POLICY_ALL) then
             call select_wanted(s, kt, errors >= s%tolerance, errors, theta, pre)
          else if (s%meth == DAV_METHOD_GJD) then
             ! the wanted pairs are solved to 1e-10 (what makes the outer iteration count equal to the reference's exact solves); the
             ! other m - lowest corrections only enrich the basis
             call gjd_correct(s, kt, min(s%lowest, kt), theta, errors)
          end if
          call grow_basis(s, kt, s%drr, pre, fun_a, fun_b)
       else
          ! 6. collapse restart (src/davidson.f90:218) and the projected matrices of the kept block (:223-226)
          call collapse_restart(s, theta, y, fun_a, fun_b)
       end if
    end do outer_loop
  end subroutine reference_policy_loop

  !> Opt-in policy "locking" (see engine_set_correction_policy; oracle/davidson_oracle.py: generalized_eigensolver_dense_locking
  !> states the same loop in the reference's building blocks).  Basis columns 1..nlock are the locked Ritz vectors (W carries
  !> their images), nlock+1..m the active basis; hm is the projected matrix of all m columns, of which only the active block is
  !> ever solved.  A contraction V <- V Z, W <- W Z (dav_restart with the m x keep matrix Z) does the locking rotation and the
  !> collapse restart in one product.  Generalized problems: basis columns 1..nlock are GUARD vectors (an orthonormal basis of
  !> span(B X_locked), see lock_and_contract); the locked eigenvectors themselves wait in the Ritz-vector panel behind its first `lowest` columns.
  subroutine davidson_locking_loop(s, max_iterations, eigenvalues, iters, done)
    type(solve_state), intent(inout) :: s
    integer, intent(in) :: max_iterations
    real(dp), intent(out) :: eigenvalues(s%lowest)
    integer, intent(inout) :: iters
    logical, intent(inout) :: done
    integer :: it, jj, nr, nc, kt, nlock, want, ma, nconv, want_new, m_rest, keep_a, keep, c0
    real(dp), allocatable :: th(:), ya(:, :), yfull(:, :), err(:), yconv(:, :)
    real(dp) :: theta_lock(s%lowest), lam(s%lowest)
    integer, allocatable :: rest(:)
    logical, allocatable :: conv(:)
    logical :: grow
    nlock = 0
    do it = 1, max_iterations
       want = s%lowest - nlock
       ma = s%m - nlock
       call check_dav(dav_agree_next(s%h, [real(it, dp), real(s%m, dp), real(nlock, dp), real(want, dp), s%tolerance, real(s%pol, dp), &
            real(s%meth, dp)], 7_c_int), "dav_agree_next")
       ! 3. Rayleigh-Ritz of the active block
       if (allocated(th)) deallocate(th, ya, yfull, err, conv)
       allocate(th(ma), ya(ma, ma), yfull(s%m, want), err(want), conv(want))
       call solve_projected(s, nlock + 1, ma, th, ya)
       call lap(s, 2)
       ! 4. Ritz vectors, residues and corrections of the pairs still wanted
       yfull = 0.0_dp
       yfull(nlock + 1:s%m, :) = ya(:, 1:want)
       call ritz_phase(s, want, want, s%meth, th, yfull, err)
       conv = err < s%tolerance
       nconv = count(conv)
       if (trace_iterations()) print "(a, i0, a, i0, a, i0, a, es10.3, a, i0)", "davidson trace (locking): iteration ", it, " m=", s%m, &
            " locked=", nlock, " max residual ", maxval(err), " newly below tolerance ", nconv
       want_new = want - nconv
       m_rest = ma - nconv
       ! rest: the active Ritz vectors that stay active, in ascending order of their values; yconv: those that converge now (ma x nconv),
       ! in the order they are locked in, their values behind the locked ones
       if (allocated(rest)) deallocate(rest, yconv)
       allocate(rest(m_rest), yconv(ma, max(nconv, 1)))
       nr = 0
       nc = 0
       do jj = 1, ma
          if (jj <= want .and. conv(min(jj, want))) then
             nc = nc + 1
             yconv(:, nc) = ya(:, jj)
             theta_lock(nlock + nc) = th(jj)
          else
             nr = nr + 1
             rest(nr) = jj
          end if
       end do
       if (want_new == 0) then
          ! every wanted pair is locked or has just converged: Ritz vectors in ascending order of the eigenvalues
          lam = theta_lock
          call assemble_locking_exit(s, nlock, lam, .true., yconv, nconv, yconv, eigenvalues)
          iters = it
          done = .true.
          return
       end if
       ! 5. the corrections of the pairs that stay wanted, compacted to the front of the block behind the basis
       kt = correction_count(s%pol, s%m, s%n, s%cap, want_new)
       call locking_rule(s%m, kt, m_rest, want_new, s%max_dim, s%cap, grow, keep_a)
       if (grow) call select_wanted(s, kt, .not. conv, err, th)
       keep = nlock + nconv + keep_a
       if (nconv > 0 .or. keep < s%m) then
          ! 6. lock what converged and contract: the locking rotation and the collapse restart in one product
          call lock_and_contract(s, nlock, nconv, keep_a, ya, rest, yconv)
          nlock = nlock + nconv
          if (grow .and. keep < s%m) then
             print *, "locking_loop: internal error (a growing iteration keeps every active Ritz vector)"
             error stop
          end if
          s%m = keep
          if (restart_is_refresh(s)) then
             ! W was contracted, not recomputed: every refresh_every-th contraction re-applies the operator (as after restarts) - to
             ! the active columns (generalized problems: the guard columns carry no images)
             c0 = merge(nlock, 0, s%gev)
             call sweep_columns(s, c0, s%m - c0)
             call project_columns(s, 0, s%m)
          end if
          call lap(s, 7)
       end if
       ! 6./7. generalized: all passes, the sweep, the plain projection (the fused last pass would read images of the guard columns)
       if (grow) call grow_basis(s, kt, s%gev)
    end do
    ! NOT CONVERGED: what is locked plus the current Ritz pairs of the active basis (the caller prints the warning).  Kept exactly as it
    ! was, ADVICE.md's finding included: yfull and ya are those of the LAST iteration, whose contraction and growth the basis has gone through
    ! since, and the vectors are only assembled when their row counts happen to fit.  The fix changes behaviour: a pull request of its own.
    lam(1:nlock) = theta_lock(1:nlock)
    if (nlock < s%lowest) lam(nlock + 1:s%lowest) = th(1:s%lowest - nlock)
    call assemble_locking_exit(s, nlock, lam, s%gev .or. size(yfull, 1) == s%m, ya, &
         merge(s%lowest - nlock, 0, size(ya, 1) == s%m - nlock), yfull, eigenvalues)
  end subroutine davidson_locking_loop

  ! ---- the rules: pure decisions, no engine calls -------------------------------------------------------------------------------------

  !> Does this iteration grow the basis or end in a collapse restart (src/davidson.f90:195), and how many Ritz pairs does its Ritz phase work
  !> on?  It only depends on the width.  The reference's policy corrects every Ritz pair, so a growing iteration needs all m eigenpairs of the
  !> projected problem; a restarting one only the 2*lowest it keeps, and the opt-in policy never more than that.
  pure subroutine growth_rule(pol, m, lowest, max_dim, cap, expand_now, ncorr)
    integer, intent(in) :: pol, m, lowest, max_dim, cap
    logical, intent(out) :: expand_now
    integer, intent(out) :: ncorr
    if (pol == POLICY_ALL) then
       expand_now = m <= max_dim
       ncorr = merge(m, lowest, expand_now)
    else
       ! grow while the widest possible block still fits; a basis that has just been (re)started always grows -
       ! as long as the projected matrices (cap x cap) can take one more column
       expand_now = ((m + lowest <= max_dim) .or. (m <= 2 * lowest)) .and. m < cap
       ncorr = lowest
    end if
  end subroutine growth_rule

  !> kt, the columns a growing iteration adds (src/davidson.f90:199: one per basis vector).  Policy all: never more than the space has left -
  !> with m + kt > n the reference stops in DORGQR (src/lapack_wrapper.f90:176-236); here the leading n - m corrections complete the basis and
  !> the next Ritz problem is exact.  The other policies: the `nwanted` pairs still wanted (cap - m: max_dim_sub < 2*lowest leaves cap = 2*lowest).
  pure function correction_count(pol, m, n, cap, nwanted) result(kt)
    integer, intent(in) :: pol, m, n, cap, nwanted
    integer :: kt
    kt = min(nwanted, n - m)
    if (pol == POLICY_ALL) kt = min(m, n - m)
    if (pol == POLICY_UNCONVERGED) kt = min(kt, cap - m)
  end function correction_count

  !> Locking: grow while the active basis (m_rest Ritz vectors stay) can take the kt corrections of the want_new pairs still wanted and the panels
  !> hold them.  keep_a, the active Ritz vectors a contraction keeps: all when the basis grows, else 2 per pair still wanted (src/davidson.f90:218)
  pure subroutine locking_rule(m, kt, m_rest, want_new, max_dim, cap, grow, keep_a)
    integer, intent(in) :: m, kt, m_rest, want_new, max_dim, cap
    logical, intent(out) :: grow
    integer, intent(out) :: keep_a
    grow = ((m_rest + want_new <= max_dim) .or. (m_rest <= 2 * want_new)) .and. (m + kt <= cap) .and. kt > 0
    keep_a = merge(m_rest, min(2 * want_new, m_rest), grow)
  end subroutine locking_rule

  ! ---- the steps ----------------------------------------------------------------------------------------------------------------------

  !> wall time since the last lap goes to phase `slot` (davidson_engine%phase_seconds)
  subroutine lap(s, slot)
    type(solve_state), intent(inout) :: s
    integer, intent(in) :: slot
    real(dp) :: t1
    t1 = tick()
    s%phase_s(slot) = s%phase_s(slot) + (t1 - s%t0)
    s%t0 = t1
  end subroutine lap

  !> Count a restart; .true. at every refresh_every-th.  W = A*V and B*V are contracted at a restart, not recomputed: each adds ~eps*|A|*sqrt(m) to
  !> W - A*V.  Re-applying the operators then, as the reference does after every restart (src/davidson.f90:223-226), bounds that drift over long runs.
  function restart_is_refresh(s) result(due)
    type(solve_state), intent(inout) :: s
    logical :: due
    s%nrestart = s%nrestart + 1
    due = mod(s%nrestart, s%refresh_every) == 0
  end function restart_is_refresh

  !> Steps 1 and 2 (src/davidson.f90:124-135).  Cold: unit vectors at the lowest diagonal entries, W0 = A*V0, the projected matrices.  Warm: the
  !> staged guess columns first, unit vectors behind them; the block is made Euclidean-orthonormal like every block that joins the basis (a
  !> B-orthonormal guess is re-orthonormalised; dependent or duplicate columns are completed by the rules of davidson_ortho), swept and projected.
  subroutine start_basis(s, warm, fun_a, fun_b)
    type(solve_state), intent(inout) :: s
    logical, intent(in) :: warm
    procedure(block_operator), optional :: fun_a, fun_b
    integer(c_int64_t) :: idx(s%m)
    integer(c_int) :: nguess
    if (warm) then
       call check_dav(dav_init_basis_guess(s%h, int(s%m, c_int), idx, nguess), "dav_init_basis_guess")
       call block_orthonormalise(s%dev, s%n, 0, s%m)
       call sweep_columns(s, 0, s%m, fun_a, fun_b)
    else
       call check_dav(dav_init_basis(s%h, int(s%m, c_int), idx), "dav_init_basis")
       if (s%host_ops) call apply_host_block(s%h, s%n, 0, s%m, fun_a, fun_b)
    end if
    call project_columns(s, 0, s%m)
  end subroutine start_basis

  !> One block sweep of the operators over basis columns [c0, c0 + k) (src/davidson.f90:223-226): on the device, and through the host callbacks
  subroutine sweep_columns(s, c0, k, fun_a, fun_b)
    type(solve_state), intent(inout) :: s
    integer, intent(in) :: c0, k
    procedure(block_operator), optional :: fun_a, fun_b
    call check_dav(dav_expand(s%h, int(c0, c_int), int(k, c_int)), "dav_expand")
    if (s%host_ops) call apply_host_block(s%h, s%n, c0, k, fun_a, fun_b)
  end subroutine sweep_columns

  !> Step 2 (src/davidson.f90:131-135, :223-227) for basis columns [c0, c0 + k): into hm / sm or, Rayleigh-Ritz on the device, the engine's copies
  subroutine project_columns(s, c0, k)
    type(solve_state), intent(inout) :: s
    integer, intent(in) :: c0, k
    if (s%drr) then
       call check_dav(dav_project_dev(s%h, int(c0, c_int), int(k, c_int)), "dav_project")
    else
       call check_dav(dav_project(s%h, int(c0, c_int), int(k, c_int), s%hm, s%ld, s%sm, s%ld), "dav_project")
    end if
  end subroutine project_columns

  !> Step 3 (src/davidson.f90:152-156): the lowest nvec eigenpairs of the block [lo, m] of the projected problem, standard or generalized, on the host
  subroutine solve_projected(s, lo, nvec, theta, y)
    type(solve_state), intent(in) :: s
    integer, intent(in) :: lo, nvec
    real(dp), intent(inout), contiguous :: theta(:), y(:, :)
    if (s%gev) then
       call lapack_rayleigh_ritz(s%hm(lo:s%m, lo:s%m), theta, y, nvec, s%sm(lo:s%m, lo:s%m))
    else
       call lapack_rayleigh_ritz(s%hm(lo:s%m, lo:s%m), theta, y, nvec)
    end if
  end subroutine solve_projected

  !> Convergence usually arrives at the widest basis, exactly where the full Ritz problem is dearest (order 64: 150-200 us on the host) although
  !> a converged iteration only needs the `lowest` wanted pairs.  When the previous residues say convergence is near, steps 3 and 4
  !> (src/davidson.f90:152-192) are made for those pairs first (MRRR on a subset) and tested; only if the test fails is the full problem solved.
  !> have_all_pairs: lapack_rayleigh_ritz solves for ALL pairs when the wanted ones are more than an eighth of the order - the caller then skips it.
  subroutine probe_wanted_pairs(s, i, expand_now, theta, y, errors, has_converged, have_all_pairs, done)
    type(solve_state), intent(inout) :: s
    integer, intent(in) :: i
    logical, intent(in) :: expand_now
    real(dp), intent(inout), contiguous :: theta(:), y(:, :)
    real(dp), intent(inout) :: errors(:)
    logical, intent(inout) :: has_converged(:), done
    logical, intent(out) :: have_all_pairs
    have_all_pairs = .false.
    if (s%drr .or. s%pol /= POLICY_ALL .or. .not. expand_now .or. i <= 1 .or. s%m < 48 .or. 2 * s%lowest > s%m) return
    if (.not. maxval(errors) < sqrt(s%tolerance)) return
    have_all_pairs = 8 * s%lowest > s%m
    call solve_projected(s, 1, s%lowest, theta, y)
    call lap(s, 2)
    call ritz_phase(s, s%lowest, s%lowest, DAV_METHOD_NONE, theta, y, errors)
    call test_convergence(s, errors, has_converged, done)
  end subroutine probe_wanted_pairs

  !> Step 4 (src/davidson.f90:158-178, and the correction of :201-206 with it): Ritz vectors, residues and their norms of the first nwant pairs,
  !> the correction `phase` for the first ncorr - one fused device phase.  With `pre`, the Gram blocks of the first orthonormalisation pass come
  !> back with the norms where the method's block is made in this phase.  Rayleigh-Ritz on the device: steps 3 + 4 there, one synchronisation.
  subroutine ritz_phase(s, ncorr, nwant, phase, theta, y, errors, pre)
    type(solve_state), intent(inout) :: s
    integer, intent(in) :: ncorr, nwant, phase
    real(dp), intent(inout), contiguous :: theta(:), y(:, :)
    real(dp), intent(inout) :: errors(:)
    type(gram_prefetch), intent(inout), target, optional :: pre
    integer(c_int) :: sweeps
    integer(c_int64_t) :: ldm
    logical :: with_gram
    ldm = int(s%m, c_int64_t)
    with_gram = .false.
    if (present(pre)) then
       with_gram = merge(method_block_in_ritz_phase(phase), phase == DAV_METHOD_DPR, s%drr)
       pre%have = with_gram
       if (with_gram .and. allocated(pre%c)) deallocate(pre%c, pre%g)
       if (with_gram) allocate(pre%c(s%m, ncorr), pre%g(ncorr, ncorr))
    end if
    if (s%drr .and. with_gram) then
       call check_dav(dav_rr_ritz(s%h, int(s%m, c_int), int(ncorr, c_int), int(nwant, c_int), int(phase, c_int), theta, &
            errors, c_loc(pre%c), ldm, c_loc(pre%g), int(ncorr, c_int64_t), sweeps), "dav_rr_ritz")
    else if (s%drr) then
       call check_dav(dav_rr_ritz(s%h, int(s%m, c_int), int(ncorr, c_int), int(nwant, c_int), int(phase, c_int), theta, &
            errors, c_null_ptr, 0_c_int64_t, c_null_ptr, 0_c_int64_t, sweeps), "dav_rr_ritz")
    else if (with_gram) then
       call check_dav(dav_ritz_residual_correction_g(s%h, int(s%m, c_int), int(ncorr, c_int), int(nwant, c_int), y, &
            ldm, theta, errors, pre%c, ldm, pre%g, int(ncorr, c_int64_t)), "dav_ritz_residual_correction")
    else
       ! (BDPR, CHEB and LCHEB too: the entry above has no method argument; the first Gram pass is then made by the orthonormalisation, as for GJD)
       call check_dav(dav_ritz_residual_correction_n(s%h, int(s%m, c_int), int(ncorr, c_int), int(nwant, c_int), y, &
            ldm, theta, int(phase, c_int), errors), "dav_ritz_residual_correction")
    end if
    call lap(s, 3)
  end subroutine ritz_phase

  !> The test of src/davidson.f90:173-178 / :189 (sticky flags) or :416 (all pairs at once)
  subroutine test_convergence(s, errors, has_converged, done)
    type(solve_state), intent(in) :: s
    real(dp), intent(in) :: errors(:)
    logical, intent(inout) :: has_converged(:)
    logical, intent(out) :: done
    done = all(errors < s%tolerance)
    if (.not. s%sticky) return
    where (errors < s%tolerance) has_converged = .true.
    done = all(has_converged)
  end subroutine test_convergence

  !> X(:, 1:lowest) = V(:, 1:m) * Y(:, 1:lowest) for the Ritz pairs of this iteration (src/davidson.f90:187; see lazy_x)
  subroutine finish_ritz_vectors(s, y)
    type(solve_state), intent(in) :: s
    real(dp), intent(in), contiguous :: y(:, :)
    if (s%lazy_x) call check_dav(dav_ritz_vectors(s%h, int(s%m, c_int), int(s%lowest, c_int), y, int(size(y, 1), c_int64_t)), &
         "dav_ritz_vectors")
  end subroutine finish_ritz_vectors

  !> The GJD correction solves of src/davidson.f90:700-734 for kt columns: the first nwanted to a wanted pair's tolerance, the others as followers
  subroutine gjd_correct(s, kt, nwanted, theta, errs)
    type(solve_state), intent(inout) :: s
    integer, intent(in) :: kt, nwanted
    real(dp), intent(in) :: theta(*), errs(*)
    real(dp) :: tols(kt)
    integer :: j
    integer(c_int) :: inner_steps          ! (comes back, is not read)
    tols = s%tol_unwanted
    do j = 1, nwanted
       tols(j) = gjd_tol_wanted(errs(j), s%tolerance, s%adaptive_c)
    end do
    call check_dav(dav_gjd_correction_n(s%h, int(s%m, c_int), int(kt, c_int), theta, 300_c_int, 1.0e-10_dp, tols, inner_steps), &
         "dav_gjd_correction")
    call lap(s, 8)
  end subroutine gjd_correct

  !> Step 5 of the opt-in policies: only the first kt pairs flagged in `still` (wanted, not converged) are corrected - their columns are compacted
  !> to the front, the others dropped.  GJD: their Ritz vectors and residues, then the solves; else: their columns of the Ritz phase's block.
  subroutine select_wanted(s, kt, still, errors, theta, pre)
    type(solve_state), intent(inout) :: s
    integer, intent(in) :: kt
    logical, intent(in) :: still(:)
    real(dp), intent(in) :: errors(:), theta(:)
    type(gram_prefetch), intent(inout), optional :: pre
    integer :: j, k
    integer(c_int) :: sel(kt)
    real(dp) :: theta_sel(kt), err_sel(kt)
    k = 0
    do j = 1, size(still)
       if (still(j) .and. k < kt) then
          k = k + 1
          sel(k) = int(j - 1, c_int)
          theta_sel(k) = theta(j)
          err_sel(k) = errors(j)
       end if
    end do
    if (s%meth == DAV_METHOD_GJD) then
       call check_dav(dav_panel_select(s%h, DAV_PANEL_X, 0_c_int, int(kt, c_int), sel), "dav_panel_select")
       call check_dav(dav_panel_select(s%h, DAV_PANEL_R, 0_c_int, int(kt, c_int), sel), "dav_panel_select")
       call gjd_correct(s, kt, kt, theta_sel, err_sel)
    else
       call check_dav(dav_panel_select(s%h, DAV_PANEL_V, int(s%m, c_int), int(kt, c_int), sel), "dav_panel_select")
       if (.not. present(pre)) return
       if (pre%have) then                                ! keep the same columns of the prefetched Gram blocks
          pre%c(:, 1:kt) = pre%c(:, sel(1:kt) + 1)
          pre%g(1:kt, 1:kt) = pre%g(sel(1:kt) + 1, sel(1:kt) + 1)
       end if
    end if
  end subroutine select_wanted

  !> Steps 6 and 7 and the projection of the new columns (src/davidson.f90:210-213, :223-227): the correction block of kt columns behind the
  !> basis is orthonormalised against V and itself, swept and projected.  Fused form: the first Gram-Schmidt pass only (the block is then
  !> orthonormal to ~1e-8), one block sweep of A over the new columns as that pass left them, and the last pass together with the projection
  !> (project_with_last_pass).  all_passes_first (device Rayleigh-Ritz, generalized locking): all passes, the device's sweep, the plain projection.
  subroutine grow_basis(s, kt, all_passes_first, pre, fun_a, fun_b)
    type(solve_state), intent(inout) :: s
    integer, intent(in) :: kt
    logical, intent(in) :: all_passes_first
    type(gram_prefetch), intent(in), optional :: pre
    procedure(block_operator), optional :: fun_a, fun_b
    logical :: have_pre
    integer :: opass
    have_pre = .false.
    if (present(pre)) have_pre = pre%have
    if (all_passes_first .and. have_pre) then
       call block_orthonormalise(s%dev, s%n, s%m, kt, pre%c(:, 1:kt), pre%g(1:kt, 1:kt))
    else if (all_passes_first) then
       call block_orthonormalise(s%dev, s%n, s%m, kt)
    else if (have_pre) then
       call block_orthonormalise(s%dev, s%n, s%m, kt, pre%c(:, 1:kt), pre%g(1:kt, 1:kt), only_first=.true., last_pass=opass)
    else
       call block_orthonormalise(s%dev, s%n, s%m, kt, only_first=.true., last_pass=opass)
    end if
    call lap(s, 4)
    if (all_passes_first) then
       call check_dav(dav_expand(s%h, int(s%m, c_int), int(kt, c_int)), "dav_expand")
       call lap(s, 5)
       call project_columns(s, s%m, kt)
    else
       call sweep_columns(s, s%m, kt, fun_a, fun_b)
       call lap(s, 5)
       call project_with_last_pass(s, kt, opass + 1, fun_a, fun_b)
    end if
    call lap(s, 6)
    s%m = s%m + kt
  end subroutine grow_basis

  !> Collapse restart: V <- V*Y(:, 1:2L) (src/davidson.f90:218).  The reference then re-applies A (and B) to the whole basis (:223-226); here W = A*V
  !> and B*V are contracted with the same columns - W*Y = A*(V*Y) to rounding: three panel products, no sweep except at a refresh (restart_is_refresh).
  subroutine collapse_restart(s, theta, y, fun_a, fun_b)
    type(solve_state), intent(inout) :: s
    real(dp), intent(inout), contiguous :: theta(:), y(:, :)
    procedure(block_operator), optional :: fun_a, fun_b
    integer :: kt
    kt = 2 * s%lowest
    if (s%drr .and. .not. s%gev) then
       call check_dav(dav_rr_restart(s%h, int(s%m, c_int), int(kt, c_int)), "dav_rr_restart")
    else
       if (s%drr) call check_dav(dav_rr_get(s%h, int(s%m, c_int), int(s%m, c_int), theta, y, int(s%m, c_int64_t)), "dav_rr_get")
       ! Y is S-orthonormal in the generalized case: V*Y(:, 1:kt) has the Gram matrix G = Y^T Y (V itself is
       ! Euclidean-orthonormal), so Y*M with M^T G M = I makes the restarted basis orthonormal again - what the
       ! reference gets from its next QR of the whole basis - and carries W and B*V along
       if (s%gev) call restart_transform(y(1:s%m, 1:kt), s%m, kt)
       call check_dav(dav_restart(s%h, int(s%m, c_int), int(kt, c_int), y, int(s%m, c_int64_t)), "dav_restart")
    end if
    if (restart_is_refresh(s)) call sweep_columns(s, 0, kt, fun_a, fun_b)
    call lap(s, 7)
    s%hm = 0.0_dp
    s%sm = 0.0_dp
    call project_columns(s, 0, kt)
    call lap(s, 6)
    s%m = kt
  end subroutine collapse_restart

  !> The last orthonormalisation pass of the block V(:, m+1:m+kt) (already swept: W, B*V hold its images) fused with the
  !> projection: dav_project_ortho returns [V T]^T (A T), [V T]^T (B T), C = V^T T and G = T^T T in one fetch; the pass
  !> T <- (T - V C) M is applied to T and its images (dav_ortho_apply_all) and to the projected blocks here:
  !>   V^T A T'' = (Hv - H C) M,   T''^T A T'' = M^T (Ht - C^T Hv - Hv^T C + C^T H C) M   (A symmetric, as everywhere).
  !> A pass that does not leave the block clean (rank-deficient corrections: rare) falls back to the separate passes, a second
  !> sweep of the block and dav_project.  (Stands for src/davidson.f90:213 and :223-227 of the new columns.)
  subroutine project_with_last_pass(s, kt, first_pass, fun_a, fun_b)
    type(solve_state), intent(inout) :: s                   !< hm, sm: their new rows / columns are filled here
    integer, intent(in) :: kt, first_pass
    procedure(block_operator), optional :: fun_a, fun_b     !< host callbacks (the matrix-free front end): the fallback path re-applies them
    integer, parameter :: max_pass = 8
    real(dp), allocatable, target :: hraw(:, :), sraw(:, :)
    real(dp), allocatable :: c2(:, :), g2(:, :), mm(:, :)
    logical, allocatable :: null_cols(:)
    real(dp) :: wmin, wmax
    type(c_ptr) :: sptr
    integer :: nnull, m, p, pass
    m = s%m
    p = m + kt
    allocate(hraw(p, kt), c2(max(m, 1), kt), g2(kt, kt), mm(kt, kt), null_cols(kt))
    sptr = c_null_ptr                                       ! generalized: the blocks of B too
    if (s%gev) allocate(sraw(p, kt))
    if (s%gev) sptr = c_loc(sraw)
    call check_dav(dav_project_ortho(s%h, int(m, c_int), int(kt, c_int), hraw, int(p, c_int64_t), sptr, &
         merge(int(p, c_int64_t), 0_c_int64_t, s%gev), c2, int(max(m, 1), c_int64_t), g2, int(kt, c_int64_t)), "dav_project_ortho")
    pass = first_pass
    do
       call ortho_pass_transform(pass, m, kt, c2, g2, mm, wmin, wmax, null_cols, nnull)
       if (nnull > 0) then
          ! numerically null columns (rank-deficient corrections: rare): they are replaced by fresh directions, which have no
          ! images yet - separate passes, a second sweep of the block and dav_project
          call block_orthonormalise(s%dev, s%n, m, kt, first_pass=pass)
          call sweep_columns(s, m, kt, fun_a, fun_b)
          call check_dav(dav_project(s%h, int(m, c_int), int(kt, c_int), s%hm, s%ld, s%sm, s%ld), "dav_project")
          return
       end if
       call check_dav(dav_ortho_apply_all(s%h, int(m, c_int), int(kt, c_int), c2, int(max(m, 1), c_int64_t), mm, &
            int(kt, c_int64_t)), "dav_ortho_apply_all")
       call transform_projected(s%hm, hraw, c2, mm, m, kt)
       if (s%gev) call transform_projected(s%sm, sraw, c2, mm, m, kt)
       if (pass >= 2 .and. wmin > 0.5_dp .and. wmax < 2.0_dp) exit          ! orthonormal to rounding
       if (pass >= max_pass) then
          print *, "Warning: block orthonormalisation did not settle in ", max_pass, " passes"
          exit
       end if
       ! one more pass (a block whose second pass still found it ill-conditioned): its Gram blocks; the images and the projected
       ! blocks keep following the block - no second sweep
       pass = pass + 1
       call check_dav(dav_ortho_gram(s%h, int(m, c_int), int(kt, c_int), c2, int(max(m, 1), c_int64_t), g2, &
            int(kt, c_int64_t)), "dav_ortho_gram")
    end do
    s%hm(1:p, m + 1:p) = hraw
    s%hm(m + 1:p, 1:m) = transpose(hraw(1:m, :))
    if (s%gev) then
       s%sm(1:p, m + 1:p) = sraw
       s%sm(m + 1:p, 1:m) = transpose(sraw(1:m, :))
    end if
  end subroutine project_with_last_pass

  !> Locking, step 6: Z = [e_1 .. e_nlock | the pairs just locked | keep_a Ritz vectors kept active], the contraction V <- V Z,
  !> W <- W Z (src/davidson.f90:218 for the active basis) and the projected matrices Z^T H Z.
  !> The Ritz vectors of a generalized problem are S-orthonormal: the kept ones are made Euclidean-orthonormal (as after a
  !> restart of the reference policy); the pairs just locked leave the basis altogether - their eigenvectors X = V_a y go to
  !> the Ritz-vector panel, and what takes their columns are their GUARD vectors B X = (B V_a) y: the pairs still wanted are
  !> B-orthogonal to the locked ones, x^T (B x_l) = 0, so the search space is kept orthogonal to span(B X_locked) instead of
  !> span(X_locked); the remaining Ritz vectors already are (y_j^T S y_l = 0).  The guard columns carry NO images (W, B V
  !> stay zero there): nothing ever projects on them - which is why the generalized loop makes its orthonormalisation
  !> passes before the sweep instead of fusing the last one with the projection, whose update reads W of every column.
  subroutine lock_and_contract(s, nlock, nconv, keep_a, ya, rest, yconv)
    type(solve_state), intent(inout) :: s
    integer, intent(in) :: nlock, nconv, keep_a, rest(:)
    real(dp), intent(in), contiguous :: ya(:, :), yconv(:, :)
    real(dp), allocatable :: z(:, :), za(:, :)
    integer :: jj, m, ma, keep
    m = s%m
    ma = m - nlock
    keep = nlock + nconv + keep_a
    allocate(z(m, keep), za(ma, keep_a))
    z = 0.0_dp
    z(1:nlock, 1:nlock) = eye(nlock, nlock)
    do jj = 1, keep_a
       za(:, jj) = ya(:, rest(jj))
    end do
    if (s%gev) then
       if (keep_a > 0) call restart_transform(za, ma, keep_a)
       if (nconv > 0) then
          call check_dav(dav_panel_transform(s%h, DAV_PANEL_V, int(nlock, c_int), int(ma, c_int), yconv, int(ma, c_int64_t), int(nconv, c_int), &
               DAV_PANEL_X, int(s%lowest + nlock, c_int)), "dav_panel_transform")
          ! (into the residue panel: the correction of this iteration has been made, nothing reads it before the next Ritz phase;
          ! the scratch panel S is what a contraction of more than 64 columns goes through - dav_restart below)
          call check_dav(dav_panel_transform(s%h, DAV_PANEL_BV, int(nlock, c_int), int(ma, c_int), yconv, int(ma, c_int64_t), int(nconv, c_int), &
               DAV_PANEL_R, 0_c_int), "dav_panel_transform")
       end if
    else
       z(nlock + 1:m, nlock + 1:nlock + nconv) = yconv(:, 1:nconv)
    end if
    z(nlock + 1:m, nlock + nconv + 1:keep) = za
    ! (a growing iteration keeps every active Ritz vector, keep = m: the correction block behind column m stays where it is)
    call check_dav(dav_restart(s%h, int(m, c_int), int(keep, c_int), z, int(m, c_int64_t)), "dav_restart")
    s%hm(1:keep, 1:keep) = lapack_matmul("T", "N", z, lapack_matmul("N", "N", s%hm(1:m, 1:m), z))
    if (s%gev) s%sm(1:keep, 1:keep) = lapack_matmul("T", "N", z, lapack_matmul("N", "N", s%sm(1:m, 1:m), z))
    if (keep < m) s%hm(keep + 1:m, :) = 0.0_dp
    if (keep < m) s%hm(:, keep + 1:m) = 0.0_dp
    if (s%gev .and. keep < m) s%sm(keep + 1:m, :) = 0.0_dp
    if (s%gev .and. keep < m) s%sm(:, keep + 1:m) = 0.0_dp
    if (s%gev .and. nconv > 0) then
       ! the guard vectors of the pairs just locked into their columns, orthonormal to the guards before them and to each other
       call check_dav(dav_panel_transform(s%h, DAV_PANEL_R, 0_c_int, int(nconv, c_int), eye(nconv, nconv), int(nconv, c_int64_t), &
            int(nconv, c_int), DAV_PANEL_V, int(nlock, c_int)), "dav_panel_transform")
       call block_orthonormalise(s%dev, s%n, nlock, nconv)
    end if
  end subroutine lock_and_contract

  !> Locking: what a solve returns when its loop stops (src/davidson.f90:186-187) - `lam` (locked values first) in ascending order and, with_vectors,
  !> the vectors in that order in the first `lowest` columns of panel X.  Generalized: the locked vectors wait behind column `lowest`; ndev more,
  !> V_active * ydev(:, 1:ndev), join them, then one permutation.  Standard: V * ysel - unit columns for the locked, yhost's columns for the others.
  subroutine assemble_locking_exit(s, nlock, lam, with_vectors, ydev, ndev, yhost, eigenvalues)
    type(solve_state), intent(inout) :: s
    integer, intent(in) :: nlock, ndev
    real(dp), intent(in) :: lam(:)
    logical, intent(in) :: with_vectors
    real(dp), intent(in), contiguous :: ydev(:, :), yhost(:, :)
    real(dp), intent(out) :: eigenvalues(:)
    real(dp) :: perm(s%lowest, s%lowest), ysel(s%m, s%lowest)
    integer :: order(s%lowest), jj
    call ascending_order(lam, order)
    eigenvalues = lam(order)
    if (.not. with_vectors) return
    if (s%gev) then
       if (ndev > 0) call check_dav(dav_panel_transform(s%h, DAV_PANEL_V, int(nlock, c_int), int(s%m - nlock, c_int), ydev, &
            int(s%m - nlock, c_int64_t), int(ndev, c_int), DAV_PANEL_X, int(s%lowest + nlock, c_int)), "dav_panel_transform")
       perm = 0.0_dp
       do jj = 1, s%lowest
          perm(order(jj), jj) = 1.0_dp
       end do
       call check_dav(dav_panel_transform(s%h, DAV_PANEL_X, int(s%lowest, c_int), int(s%lowest, c_int), perm, &
            int(s%lowest, c_int64_t), int(s%lowest, c_int), DAV_PANEL_X, 0_c_int), "dav_panel_transform")
    else
       ysel = 0.0_dp
       do jj = 1, s%lowest
          if (order(jj) <= nlock) then
             ysel(order(jj), jj) = 1.0_dp
          else if (order(jj) - nlock <= size(yhost, 2)) then
             ysel(s%m - size(yhost, 1) + 1:, jj) = yhost(:, order(jj) - nlock)
          end if
       end do
       call check_dav(dav_ritz_vectors(s%h, int(s%m, c_int), int(s%lowest, c_int), ysel, int(s%m, c_int64_t)), "dav_ritz_vectors")
    end if
  end subroutine assemble_locking_exit

  subroutine device_ortho_gram(be, m, kt, c, g)
    class(device_ortho), intent(inout) :: be
    integer, intent(in) :: m, kt
    real(dp), intent(out) :: c(:, :), g(:, :)
    call check_dav(dav_ortho_gram(be%h, int(m, c_int), int(kt, c_int), c, int(size(c, 1), c_int64_t), g, int(size(g, 1), c_int64_t)), &
         "dav_ortho_gram")
  end subroutine device_ortho_gram

  subroutine device_ortho_apply(be, m, kt, c, mm)
    class(device_ortho), intent(inout) :: be
    integer, intent(in) :: m, kt
    real(dp), intent(in) :: c(:, :), mm(:, :)
    call check_dav(dav_ortho_apply(be%h, int(m, c_int), int(kt, c_int), c, int(size(c, 1), c_int64_t), mm, int(size(mm, 1), c_int64_t)), &
         "dav_ortho_apply")
  end subroutine device_ortho_apply

  function device_ortho_unit_column(be, m, j, entry) result(ok)
    class(device_ortho), intent(inout) :: be
    integer, intent(in) :: m, j, entry
    logical :: ok
    integer(c_int) :: ierr
    ierr = dav_panel_unit_column(be%h, DAV_PANEL_V, int(m + j - 1, c_int), int(entry, c_int))
    ! DAV_NO_SUCH_ENTRY: the engine keeps no such entry of the start order - the caller takes another direction; anything else is an error
    if (ierr /= 0_c_int .and. ierr /= DAV_NO_SUCH_ENTRY) call check_dav(ierr, "dav_panel_unit_column")
    ok = ierr == 0_c_int
  end function device_ortho_unit_column

  subroutine device_ortho_put_column(be, m, j, vec)
    class(device_ortho), intent(inout) :: be
    integer, intent(in) :: m, j
    real(dp), intent(in) :: vec(:)
    call check_dav(dav_panel_put(be%h, DAV_PANEL_V, int(m + j - 1, c_int), 1_c_int, vec, int(size(vec), c_int64_t)), "dav_panel_put")
  end subroutine device_ortho_put_column

  !> Apply host callbacks to basis columns c0+1..c0+k: download the block, call, upload A*V and B*V.
  subroutine apply_host_block(h, n, c0, k, fun_a, fun_b)
    type(c_ptr), intent(in) :: h
    integer, intent(in) :: n, c0, k
    procedure(block_operator) :: fun_a, fun_b
    real(dp), allocatable :: blk(:, :), img(:, :)
    allocate(blk(n, k), img(n, k))
    call check_dav(dav_panel_get(h, DAV_PANEL_V, int(c0, c_int), int(k, c_int), blk, int(n, c_int64_t)), &
         "dav_panel_get")
    img = fun_a(blk)
    call check_dav(dav_panel_put(h, DAV_PANEL_W, int(c0, c_int), int(k, c_int), img, int(n, c_int64_t)), &
         "dav_panel_put")
    img = fun_b(blk)
    call check_dav(dav_panel_put(h, DAV_PANEL_BV, int(c0, c_int), int(k, c_int), img, int(n, c_int64_t)), &
         "dav_panel_put")
  end subroutine apply_host_block

end module davidson_loop
