"""CPU: the C ABI is written down four times - the two headers, the ctypes prototype tables of fortran_davidson_amd/_abi.py, the
Fortran interface module davidson_hip_c.f90 and the bind(C) doors of davidson_c_api.f90 - and this module reads all of them as text
and fails, naming the entry, when one drifts from the headers.  Nothing is compiled, loaded onto a GPU or run.

A signature is (return class, (argument class, ...)) with the classes "ptr" (anything passed as an address), "i32", "i64", "u64",
"f64", and for returns also "str" (const char*) and "void" (a Fortran subroutine).  size_t is "u64" (LP64).  Fortran has no unsigned
kinds and returns a string as type(c_ptr), so its side is compared with "u64" read as "i64" and "str" as "ptr"."""
import ctypes as C
import os
import re

import pytest

from fortran_davidson_amd import _abi, engine_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC_H = os.path.join(ROOT, "include", "davidson_hip.h")
PRIVATE_H = os.path.join(ROOT, "fortran_davidson_amd", "csrc", "davidson_hip_private.h")
HIP_C_F90 = os.path.join(ROOT, "fortran_davidson_amd", "fortran", "davidson_hip_c.f90")
C_API_F90 = os.path.join(ROOT, "fortran_davidson_amd", "fortran", "davidson_c_api.f90")

C_SCALARS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint64_t": "u64", "size_t": "u64", "double": "f64"}
C_POINTER_TYPEDEFS = ("dav_handle_t", "dav_device_apply_fn")
CTYPES = {C.c_void_p: "ptr", C.c_int: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_size_t: "u64", C.c_double: "f64",
          C.c_char_p: "str", None: "void"}
F_VALUE_KINDS = {"integer(c_int)": "i32", "integer(c_int32_t)": "i32", "integer(c_int64_t)": "i64", "integer(c_size_t)": "i64",
                 "real(c_double)": "f64", "type(c_ptr)": "ptr", "type(c_funptr)": "ptr"}


def read(path):
    with open(path) as f:
        return f.read()


def strip_c_comments(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def c_class(decl):
    """class of one C parameter or return type, e.g. "const double* a" -> "ptr", "int64_t lda" -> "i64" """
    words = [w for w in re.findall(r"\w+|\*", decl) if w != "const"]
    if "*" in words or words[0] in C_POINTER_TYPEDEFS:
        return "ptr"
    return C_SCALARS[words[0]]


def header_prototypes(text):
    """name -> signature of every `ret dav_name(args);` of a header"""
    out = {}
    for ret, name, args in re.findall(r"\b(const\s+char\s*\*|int)\s+(dav_\w+)\s*\(([^()]*)\)\s*;", strip_c_comments(text)):
        args = [a.strip() for a in args.split(",")]
        out[name] = ("str" if "*" in ret else "i32", () if args == ["void"] else tuple(c_class(a) for a in args))
    return out


def header_stats_fields(text):
    """[(field, C type)] of typedef struct dav_stats, in order"""
    body = re.search(r"typedef\s+struct\s+dav_stats\s*\{(.*?)\}\s*dav_stats\s*;", strip_c_comments(text), flags=re.S).group(1)
    return [(name.strip(), ctype) for ctype, names in re.findall(r"(\w+)\s+([^;]+);", body) for name in names.split(",")]


def table_signatures(table):
    return {name: (CTYPES[restype], tuple(CTYPES[a] for a in argtypes)) for name, (restype, argtypes) in table.items()}


def fortran_procedures(text, prefix):
    """name -> signature of every procedure with bind(C, name="<prefix>...") in a Fortran source: interface bodies and module procedures
    alike.  A dummy with the value attribute has the class of its kind; every other dummy is passed by reference: "ptr"."""
    lines, pending = [], ""
    for raw in text.splitlines():
        line = pending + raw.split("!")[0].strip()
        pending = line[:-1] if line.endswith("&") else ""
        if not pending and line:
            lines.append(line.lower())
    out, i = {}, 0
    while i < len(lines):
        head = re.match(r"(subroutine|function)\s+\w+\s*\(([^)]*)\)(.*)", lines[i])
        bound = head and re.search(r'bind\(c,\s*name="(\w+)"\)', head.group(3))
        i += 1
        if not bound or not bound.group(1).startswith(prefix):
            continue
        dummies = [d.strip() for d in head.group(2).split(",") if d.strip()]
        result = re.search(r"result\((\w+)\)", head.group(3))
        declared = {}
        while not re.match(r"end\b", lines[i]) and not lines[i].startswith("contains"):
            decl = re.match(r"((?:integer|real|type|character)\([^)]*\))([^:]*)::(.*)", lines[i])
            if decl:
                kind, value = decl.group(1).replace(" ", ""), "value" in [a.strip() for a in decl.group(2).split(",")]
                for var in re.sub(r"\([^()]*\)", "", decl.group(3)).split(","):
                    declared.setdefault(var.split("=")[0].strip(), F_VALUE_KINDS[kind] if value else (kind, "ptr"))
            i += 1
        args = tuple(declared[d] if isinstance(declared[d], str) else "ptr" for d in dummies)
        ret = "void" if head.group(1) == "subroutine" else F_VALUE_KINDS[declared[result.group(1)][0]]
        out[bound.group(1)] = (ret, args)
    return out


def as_fortran_sees(sig):
    ret, args = sig
    return ("ptr" if ret == "str" else ret, tuple("i64" if a == "u64" else a for a in args))


def mismatches(want, have, exact_names=True, see=lambda sig: sig):
    """every way `have` differs from `want` (both name -> signature), one line each and the entry named; exact_names=False: `have`
    may hold fewer entries than `want` (the Fortran module binds what the driver needs), but none that `want` lacks"""
    out = [f"{name}: not declared" for name in sorted(set(have) - set(want))]
    if exact_names:
        out += [f"{name}: missing" for name in sorted(set(want) - set(have))]
    for name in sorted(set(want) & set(have)):
        (wret, wargs), (hret, hargs) = see(want[name]), have[name]
        if wret != hret:
            out.append(f"{name}: returns {hret}, declared {wret}")
        if len(wargs) != len(hargs):
            out.append(f"{name}: takes {len(hargs)} arguments, declared {len(wargs)}")
            continue
        out += [f"{name}: argument {k} is {h}, declared {w}" for k, (w, h) in enumerate(zip(wargs, hargs)) if w != h]
    return out


@pytest.fixture(scope="module")
def header():
    public, private = header_prototypes(read(PUBLIC_H)), header_prototypes(read(PRIVATE_H))
    assert len(public) == 75 and len(private) == 12 and not set(public) & set(private)
    return {**public, **private}


def test_ctypes_prototypes_equal_the_headers(header):
    """_abi.DAV: exactly the headers' names, and for each the return type and every argument's class and width"""
    assert mismatches(header, table_signatures(_abi.DAV)) == []
    assert C.sizeof(C.c_size_t) == 8 and C.sizeof(C.c_int) == 4          # what the classes above assume
    assert set(_abi.TEST_BUILD_ONLY) <= set(header_prototypes(read(PRIVATE_H)))


def test_fortran_interfaces_equal_the_header(header):
    """every interface body name="dav_*" of davidson_hip_c.f90: arity, the kind of every value scalar, and a pointer of the header is
    a dummy passed by reference or a type(c_ptr) / type(c_funptr) value"""
    bound = fortran_procedures(read(HIP_C_F90), "dav_")
    assert len(bound) == 67
    assert mismatches(header, bound, exact_names=False, see=as_fortran_sees) == []


def test_ctypes_prototypes_equal_the_fortran_doors():
    """_abi.FD against the bind(C, name="fd_*") procedures of davidson_c_api.f90, the same way"""
    doors = fortran_procedures(read(C_API_F90), "fd_")
    assert len(doors) == 41
    assert mismatches(doors, table_signatures(_abi.FD)) == []


def test_every_entry_the_package_calls_is_declared():
    """a dav_* / fd_* call of the Python layer that the tables lack would run without a prototype"""
    pkg = os.path.join(ROOT, "fortran_davidson_amd")
    called = {name for f in os.listdir(pkg) if f.endswith(".py") for name in re.findall(r"\.((?:dav|fd)_\w+)\(", read(os.path.join(pkg, f)))}
    assert len(called) > 100 and called <= set(_abi.DAV) | set(_abi.FD)


def test_stats_mirror_and_abi_version_equal_the_header():
    text = read(PUBLIC_H)
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    assert engine_c.Stats._fields_ == [(name, ctype[t]) for name, t in header_stats_fields(text)]
    assert engine_c.ABI_VERSION == int(re.search(r"#define\s+DAV_HIP_ABI_VERSION\s+(\d+)", text).group(1))


def test_the_checker_names_a_changed_width_and_a_removed_prototype(header):
    """the comparison can fail: one int parameter of the header made int64_t, then one prototype taken out - each is reported, by name,
    against the table and against the Fortran module"""
    text = read(PUBLIC_H)
    bound = fortran_procedures(read(HIP_C_F90), "dav_")
    table = table_signatures(_abi.DAV)
    private = header_prototypes(read(PRIVATE_H))

    widened = text.replace("int dav_expand(dav_handle_t h, int m, int kt);", "int dav_expand(dav_handle_t h, int m, int64_t kt);")
    assert widened != text
    changed = {**header_prototypes(widened), **private}
    assert mismatches(changed, table) == ["dav_expand: argument 2 is i32, declared i64"]
    assert mismatches(changed, bound, exact_names=False, see=as_fortran_sees) == ["dav_expand: argument 2 is i32, declared i64"]

    removed = re.sub(r"int dav_expand\([^;]*;", "", text)
    assert removed != text
    changed = {**header_prototypes(removed), **private}
    assert len(changed) == len(header) - 1
    assert mismatches(changed, table) == ["dav_expand: not declared"]
    assert mismatches(changed, bound, exact_names=False, see=as_fortran_sees) == ["dav_expand: not declared"]
    assert mismatches(header, {k: v for k, v in table.items() if k != "dav_expand"}) == ["dav_expand: missing"]


def test_a_scalar_wrapped_in_the_wrong_type_raises():
    """dav_panel_get takes its leading dimension as int64_t: a c_int there fails in the conversion, before the library is reached
    (null handle, never used)"""
    from fortran_davidson_amd._lib import hip_lib
    buf = (C.c_double * 4)()
    with pytest.raises(C.ArgumentError):
        hip_lib().dav_panel_get(None, 0, 0, 1, buf, C.c_int(4))
