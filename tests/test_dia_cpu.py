"""No GPU: the storage by diagonals of a CSR operator (DAV_CSR_DIAGONALS) in the mirrors of the interface - the header and the Fortran
parameter, the component of csr_matrix, the flag word the Python layer builds - and the eligibility rule of the numpy restatement that
the GPU tests compare the engine with."""
import inspect
import os
import re

import numpy as np

import fortran_davidson_amd as fd
from fortran_davidson_amd import engine_c, solver
import cheb_inputs
import dia_inputs as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_header_and_the_fortran_parameter_agree_on_the_flag():
    hdr = read("include", "davidson_hip.h")
    m = re.search(r"enum\s*\{\s*DAV_CSR_FULL = 0,\s*DAV_CSR_LOWER = 1,\s*DAV_CSR_DIAGONALS = (\d+)", hdr)
    assert m and int(m.group(1)) == 2
    f90 = read("fortran_davidson_amd", "fortran", "davidson_hip_c.f90")
    m = re.search(r"integer\(c_int\), parameter :: DAV_CSR_DIAGONALS = (\d+)", f90)
    assert m and int(m.group(1)) == 2
    assert engine_c.CSR_DIAGONALS == 2 == D.CSR_DIAGONALS
    assert "DIA_MAX_FILL = 4" in hdr
    assert re.search(r"DAV_KIND_DIA = 9", read("fortran_davidson_amd", "csrc", "common.h"))
    assert "constexpr int DIA_MAX_FILL = 4;" in read("fortran_davidson_amd", "csrc", "dia_rule.h")


def test_csr_matrix_has_the_component_and_the_constructor_takes_it():
    f90 = read("fortran_davidson_amd", "fortran", "davidson_sparse.f90")
    body = f90[f90.index("type :: csr_matrix"):f90.index("end type csr_matrix")]
    assert re.search(r"logical :: diagonals = \.false\.", body)
    assert re.search(r"function new_csr_matrix\(n, row_ptr, col_idx, values, lower, diagonals\)", f90)
    # the device entry keeps its positions: the new argument comes behind the old ones
    assert re.search(r"subroutine engine_set_sparse_device\(eng, which, n, row_ptr, col_idx, vals, base, lower, row_ptr_bits, col_bits, stat, "
                     r"diagonals\)", f90)
    api = read("fortran_davidson_amd", "fortran", "davidson_c_api.f90")
    assert "a%diagonals = iand(lower, DAV_CSR_DIAGONALS) /= 0" in api


def test_the_python_layer_builds_the_flag_word():
    assert [engine_c.csr_flag_word(lo, di) for lo in (False, True) for di in (False, True)] == [0, 2, 1, 3]
    assert [D.flag_word(lo, di) for lo in (False, True) for di in (False, True)] == [0, 2, 1, 3]
    for fn in (fd.CEngine.set_operator_csr, fd.CEngine.set_operator_csr_dev, solver.DavidsonEngine.set_sparse,
               solver.generalized_eigensolver_sparse):
        assert inspect.signature(fn).parameters["diagonals"].default is False, fn


def test_the_rule_accepts_stencils_and_refuses_a_random_pattern():
    n = 50
    tri = np.diag(np.full(n, 2.0)) - np.eye(n, k=1) - np.eye(n, k=-1)
    rows, cols, _ = D.canonical(n, *D.csr_of_dense(tri))
    assert D.offsets(rows, cols).tolist() == [-1, 0, 1] and D.eligible(3, n, rows.size)
    n7, r7, c7, v7 = D.pattern("stencil")
    rows, cols, _ = D.canonical(n7, *D.csr_form(n7, r7, c7, v7))
    assert D.offsets(rows, cols).tolist() == [-49, -7, -1, 0, 1, 7, 49] and D.eligible(7, n7, rows.size)
    a = cheb_inputs.random_sparse(301, 6 / 301, 1)
    rows, cols, _ = D.canonical(301, *D.csr_of_dense(a))
    nd = D.offsets(rows, cols).size
    assert nd > 100 and not D.eligible(nd, 301, rows.size)


def test_lower_and_full_input_have_the_same_canonical_matrix_and_slots():
    for name in D.PATTERNS:
        n, r, c, v = D.pattern(name)
        full = D.canonical(n, *D.csr_form(n, r, c, v))
        low = D.canonical(n, *D.csr_form(n, r, c, v, lower=True, base=1), lower=True, base=1)
        offs = D.offsets(full[0], full[1])
        assert np.array_equal(offs, D.offsets(low[0], low[1])), name
        sf, sl = D.slots(n, *full, offs), D.slots(n, *low, offs)
        assert np.array_equal(sf, sl), name
        dense = np.zeros((n, n))
        np.add.at(dense, (r, c), v)
        x = np.random.default_rng(0).integers(-5, 6, (n, 3)).astype(np.float64)
        assert np.array_equal(D.dia_product(n, offs, sf, x), dense @ x), name
