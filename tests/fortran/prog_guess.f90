!> Warm start from Fortran: a dense matrix is solved cold; its eigenvectors are then handed back as initial_vectors= through the dense
!> specific and through a resident engine (engine_set_initial_vectors, engine_keep_result_as_guess), and a positional call with the
!> reference's argument list still compiles and behaves as before.  Prints "CHECK name T|F" lines and stops with a non-zero code on
!> any F.
program prog_guess
  use iso_c_binding
  use numeric_kinds, only: dp
  use davidson, only: generalized_eigensolver, engine_set_initial_vectors, engine_set_initial_vectors_device, engine_keep_result_as_guess
  use davidson_device
  implicit none
  integer, parameter :: n = 300, lowest = 3
  real(dp) :: a(n, n), ev_cold(lowest), ev_warm(lowest), ev_eng(lowest), ev_keep(lowest), ev_pos(lowest), ev_eng_cold(lowest)
  real(dp) :: x_cold(n, lowest), x(n, lowest)
  type(davidson_engine) :: eng
  integer :: it_cold, it_warm, it_eng, it_keep, it_pos, it_eng_cold, i, j, nfail, stat

  nfail = 0
  a = 0.0_dp
  do i = 1, n
     a(i, i) = real(i, dp)
     do j = max(1, i - 3), i - 1
        a(i, j) = 0.05_dp / real(i - j, dp)
        a(j, i) = a(i, j)
     end do
  end do

  ! the reference's positional argument list (src/davidson.f90:51-52), cold
  call generalized_eigensolver(a, ev_cold, x_cold, lowest, "DPR", 100, 1d-8, it_cold, 10 * lowest)
  call generalized_eigensolver(a, ev_pos, x, lowest, "DPR", 100, 1d-8, it_pos)
  call check("positional_calls_agree", all(ev_pos == ev_cold) .and. it_pos == it_cold .and. it_cold > 1)

  ! the same call with the converged vectors as the guess
  call generalized_eigensolver(a, ev_warm, x, lowest, "DPR", 100, 1d-8, it_warm, 10 * lowest, initial_vectors=x_cold)
  call check("dense_initial_vectors", it_warm == 1 .and. maxval(abs(ev_warm - ev_cold)) < 1d-8)

  ! a resident engine: a one-shot guess, then the result kept as the guess of the next solve
  call engine_create(eng, n, lowest, 10 * lowest, gev=.false.)
  call engine_set_dense(eng, 1, a)
  call generalized_eigensolver(eng, ev_eng_cold, x, lowest, "DPR", 100, 1d-8, it_eng_cold, 10 * lowest)
  call engine_keep_result_as_guess(eng, .false.)            ! (the default, said aloud: the cold solve's vectors are not reused)
  call engine_set_initial_vectors(eng, x_cold)
  call generalized_eigensolver(eng, ev_eng, x, lowest, "DPR", 100, 1d-8, it_eng, 10 * lowest)
  call check("engine_set_initial_vectors", it_eng == 1 .and. maxval(abs(ev_eng - ev_cold)) < 1d-8)
  call engine_keep_result_as_guess(eng, .true.)
  call generalized_eigensolver(eng, ev_keep, x, lowest, "DPR", 100, 1d-8, it_keep, 10 * lowest)
  call check("engine_keep_result_as_guess", it_keep == 1 .and. maxval(abs(ev_keep - ev_cold)) < 1d-8)
  call engine_keep_result_as_guess(eng, .false.)
  call generalized_eigensolver(eng, ev_keep, x, lowest, "DPR", 100, 1d-8, it_keep, 10 * lowest, initial_vectors=x_cold)
  call check("engine_initial_vectors_keyword", it_keep == 1)
  ! a null pointer is refused with a status, and the engine stays usable
  call engine_set_initial_vectors_device(eng, c_null_ptr, n, lowest, stat)
  call check("device_entry_refuses_null", stat /= 0)
  call generalized_eigensolver(eng, ev_keep, x, lowest, "DPR", 100, 1d-8, it_keep, 10 * lowest)
  call check("cold_again", it_keep == it_eng_cold .and. it_eng_cold > 1 .and. all(ev_keep == ev_eng_cold) .and. &
       maxval(abs(ev_keep - ev_cold)) < 1d-8)
  call engine_destroy(eng)

  print "(a, 6i6)", "ITERS", it_cold, it_warm, it_eng, it_keep, it_pos, it_eng_cold
  if (nfail > 0) error stop 1

contains

  subroutine check(name, ok)
    character(len=*), intent(in) :: name
    logical, intent(in) :: ok
    print "(a, 1x, a, 1x, l1)", "CHECK", name, ok
    if (.not. ok) nfail = nfail + 1
  end subroutine check

end program prog_guess
