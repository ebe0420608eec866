!> The correction methods of the driver: their names, their codes (include/davidson_hip.h) and what the loop asks of a code.  Everything
!> about method names and codes lives here; a new method is one row in `methods` and, where it applies, in method_block_in_ritz_phase.
module davidson_method
  use, intrinsic :: iso_c_binding, only: c_int
  implicit none
  private
  public :: DAV_METHOD_DPR, DAV_METHOD_GJD, DAV_METHOD_NONE, DAV_METHOD_BDPR, DAV_METHOD_CHEB, DAV_METHOD_LCHEB, &
       method_code, method_label, method_kind, method_block_in_ritz_phase, unknown_method_message

  !> DAV_METHOD_NONE: residues and norms only (the iteration will restart), not a name a caller can give.  BDPR: block-diagonal DPR for
  !> BSR operators.  CHEB: the Chebyshev-filtered correction for CSR / BSR operators; LCHEB: the same correction with a Lanczos bound,
  !> for any operator the engine applies on the device.  The code of these two sits in the low byte of the integer the engine takes,
  !> the degree (1..64, 0 = the engine's default) above it.  (All opt-in, none in the reference.)
  integer(c_int), parameter :: DAV_METHOD_DPR = 0, DAV_METHOD_GJD = 1, DAV_METHOD_NONE = 2, DAV_METHOD_BDPR = 3, DAV_METHOD_CHEB = 4, &
       DAV_METHOD_LCHEB = 5

  type :: method_row
     character(len=5) :: name
     integer :: code
     logical :: takes_degree      !< "<name><d>" with 1 <= d <= 64 is code + 256 d (the header's DAV_METHOD_CHEB_DEGREE / _LCHEB_DEGREE)
  end type method_row
  type(method_row), parameter :: methods(5) = [ &
       method_row("DPR  ", DAV_METHOD_DPR, .false.), method_row("GJD  ", DAV_METHOD_GJD, .false.), &
       method_row("BDPR ", DAV_METHOD_BDPR, .false.), method_row("CHEB ", DAV_METHOD_CHEB, .true.), &
       method_row("LCHEB", DAV_METHOD_LCHEB, .true.)]

contains

  !> the code of a method name: a name of `methods`, or one that takes a degree followed by one or two digits that say 1..64; anything
  !> else -> -1
  function method_code(name) result(code)
    character(len=*), intent(in) :: name
    integer :: code, i, j, l, d, stat
    code = -1
    do i = 1, size(methods)
       l = len_trim(methods(i)%name)
       if (len_trim(name) < l) cycle
       if (name(1:l) /= methods(i)%name(1:l)) cycle
       if (len_trim(name) == l) then
          code = methods(i)%code
          return
       end if
       if (.not. methods(i)%takes_degree .or. len_trim(name) > l + 2) cycle
       do j = l + 1, len_trim(name)
          if (index("0123456789", name(j:j)) == 0) return
       end do
       read (name(l + 1:len_trim(name)), *, iostat=stat) d
       if (stat /= 0) return
       if (d >= 1 .and. d <= 64) code = methods(i)%code + 256 * d
       return
    end do
  end function method_code

  !> what the driver prints before it stops on a name method_code does not know
  function unknown_method_message(name) result(msg)
    character(len=*), intent(in) :: name
    character(len=:), allocatable :: msg
    msg = "generalized_eigensolver: unknown correction method '" // name // "' (DPR, GJD or BDPR)" // &
         ", or CHEB / CHEB<degree 1..64>" // ", or LCHEB / LCHEB<degree 1..64>"
  end function unknown_method_message

  !> the method of a method code, as the engine splits it (csrc/engine_internal.h: parse_method): the low byte where that is CHEB or
  !> LCHEB and the code is positive - the degree rides above it -, every other code is its own method
  pure function method_kind(code) result(kind)
    integer, intent(in) :: code
    integer :: kind
    kind = code
    if (code > 0 .and. (iand(code, 255) == DAV_METHOD_CHEB .or. iand(code, 255) == DAV_METHOD_LCHEB)) kind = iand(code, 255)
  end function method_kind

  !> the inverse of method_code - what the bind(C) doors hand to generalized_eigensolver: the name, and behind one that takes a degree the
  !> degree of the code ("CHEB16"; none = the default degree).  A degree the driver does not take (outside 1..64) makes a name it does
  !> not know, and so does a code that names no method: "XXX" (a negative code has always been "DPR").
  function method_label(code) result(label)
    integer(c_int), intent(in) :: code
    character(len=12) :: label
    integer :: i, l
    label = "XXX"
    if (code < 0) label = "DPR"
    do i = 1, size(methods)
       if (method_kind(int(code)) /= methods(i)%code) cycle
       label = methods(i)%name
       l = len_trim(label)
       if (methods(i)%takes_degree .and. ishft(code, -8) /= 0) write (label(l + 1:12), "(i0)") ishft(code, -8)
    end do
  end function method_label

  !> The correction block comes out of the Ritz phase (the engine's block_in_ritz_phase): DPR, and like it BDPR, CHEB and LCHEB - wherever
  !> the loop asks for GJD these take the DPR side; the engine refuses operators a method does not serve.  GJD's block is made behind the
  !> phase, from X and R; DAV_METHOD_NONE has none.
  pure function method_block_in_ritz_phase(code) result(yes)
    integer, intent(in) :: code
    logical :: yes
    integer :: kind
    kind = method_kind(code)
    yes = kind == DAV_METHOD_DPR .or. kind == DAV_METHOD_BDPR .or. kind == DAV_METHOD_CHEB .or. kind == DAV_METHOD_LCHEB
  end function method_block_in_ritz_phase

end module davidson_method
