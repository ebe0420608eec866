!> The table of correction methods as the Fortran driver and the bind(C) doors see it (module davidson_method), for
!> tests/test_methods_cpu.py: one line "NAME [<name>] <method_code> [<method_label of it>] <method_kind> <block in the Ritz phase>" per
!> name, one line "CODE <code> [<method_label>] <method_kind>" per raw code, then what the driver prints before it stops on a name it
!> does not know, printed as the driver prints it.  Needs no GPU.
program prog_methods
  use iso_c_binding, only: c_int
  use davidson_method
  implicit none
  character(len=8), parameter :: names(26) = [character(len=8) :: "DPR", "GJD", "BDPR", "CHEB", "CHEB1", "CHEB16", "CHEB64", "CHEB0", &
       "CHEB65", "CHEBx", "CHEB-1", "CHEB1.5", "CHEB 4", "LCHEB", "LCHEB1", "LCHEB16", "LCHEB64", "LCHEB0", "LCHEB65", "LCHEBx", &
       "LCHEB123", "LCHE", "nonsense", "", "dpr", "Cheb"]
  integer, parameter :: codes(14) = [0, 1, 2, 3, 4, 5, 6, 255, 256, 260, 1282, 4100, 4101, 16644]
  integer :: i, code
  do i = 1, size(names)
     code = method_code(trim(names(i)))
     print "(3a, i0, 3a, i0, 1x, l1)", "NAME [", trim(names(i)), "] ", code, " [", trim(method_label(int(code, c_int))), "] ", &
          method_kind(code), method_block_in_ritz_phase(code)
  end do
  do i = 1, size(codes)
     print "(a, i0, 3a, i0)", "CODE ", codes(i), " [", trim(method_label(int(codes(i), c_int))), "] ", method_kind(codes(i))
  end do
  if (method_kind(method_code("LCHEB16")) /= DAV_METHOD_LCHEB) error stop "method_kind"
  print "(a)", "MESSAGE"
  print *, unknown_method_message("FOO")
end program prog_methods
