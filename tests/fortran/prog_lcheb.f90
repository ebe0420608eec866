!> The method names of the Chebyshev correction with a Lanczos bound as the Fortran driver parses them (davidson_knobs:
!> lcheb_method_code next to cheb_method_code): one line "CODE <name> <lcheb code> <cheb code>" per name, -1 = not such a name.
!> Needs no GPU (tests/test_lcheb_cpu.py).
program prog_lcheb
  use davidson_knobs, only: lcheb_method_code, cheb_method_code, method_kind, DAV_METHOD_LCHEB
  implicit none
  character(len=8), parameter :: names(12) = [character(len=8) :: "LCHEB", "LCHEB16", "LCHEB1", "LCHEB64", "LCHEB0", "LCHEB65", "LCHEBx", &
       "LCHEB123", "CHEB", "CHEB16", "LCHE", "DPR"]
  integer :: i
  do i = 1, size(names)
     print "(a, 1x, a, 1x, i0, 1x, i0)", "CODE", trim(names(i)), lcheb_method_code(trim(names(i))), cheb_method_code(trim(names(i)))
  end do
  if (method_kind(lcheb_method_code("LCHEB16")) /= DAV_METHOD_LCHEB) error stop "method_kind"
end program prog_lcheb
