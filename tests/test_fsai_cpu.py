"""CPU: the preconditioner the engine builds (davp_build_fsai) exists in every layer.  Its entries are extension entries next to ABI 109
(include/davidson_hip_precond.h, prefix davp_; doors prefix fdp_): both builds of the engine export exactly the three entries and the
Fortran library the two doors; the four mirrors - header, ctypes tables, Fortran interface module, doors - are compared the way
tests/test_herm_cpu.py compares its own; the ABI stays 109.  The numpy restatement of the build
(tests/fsai_inputs.py) agrees with numpy.linalg.solve row by row within the bound the GPU tests use, the restated solve with M = G^T G
meets the inequality the GPU solves are held to (so that it cannot pass trivially there), and no input of the GPU tests has a pattern row
of more than 64 columns except the one made for the refusal."""
import os
import re
import subprocess

import numpy as np
import pytest

import fortran_davidson_amd as fd
import fsai_inputs as F
import precond_inputs as P
from fortran_davidson_amd import _abi
from test_abi_cpu import C_API_F90, HIP_C_F90, as_fortran_sees, c_class, fortran_procedures, mismatches, read, strip_c_comments, table_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fortran_davidson_amd", "lib")
PRECOND_H = os.path.join(ROOT, "include", "davidson_hip_precond.h")
ENTRIES = {"davp_build_fsai", "davp_fsai_info", "davp_fsai_get_factor"}
DOORS = {"fdp_engine_build_fsai", "fdp_engine_fsai_info"}


def exported(lib, prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return set(re.findall(rf"\s[TW]\s+({prefix}\w+)$", out, re.M))


def precond_prototypes():
    return {name: ("i32", tuple(c_class(a.strip()) for a in args.split(",")))
            for name, args in re.findall(r"\bint\s+(davp_\w+)\s*\(([^()]*)\)\s*;", strip_c_comments(read(PRECOND_H)))}


def test_both_libraries_export_the_entries_and_the_doors():
    for lib in (os.path.join(LIBDIR, "libdavidson_hip.so"), os.path.join(LIBDIR, "test", "libdavidson_hip.so")):
        assert exported(lib, "davp_") == ENTRIES, lib
    assert exported(os.path.join(LIBDIR, "libfortran_davidson_amd.so"), "fdp_") == DOORS
    syms = subprocess.run(["strings", os.path.join(LIBDIR, "libdavidson_hip.so")], capture_output=True, text=True, check=True).stdout
    for kernel in ("fsai_pattern1_kernel", "fsai_pattern_next_kernel", "fsai_rows_kernel"):
        assert kernel in syms, kernel


def test_the_four_mirrors_are_equal():
    header = precond_prototypes()
    assert set(header) == ENTRIES
    assert header["davp_build_fsai"] == ("i32", ("ptr", "f64", "i32"))
    assert header["davp_fsai_info"] == ("i32", ("ptr", "ptr", "ptr", "ptr"))
    assert header["davp_fsai_get_factor"] == ("i32", ("ptr", "i32", "ptr", "ptr", "ptr"))
    assert mismatches(header, table_signatures(_abi.PRECOND)) == []
    assert mismatches(header, fortran_procedures(read(HIP_C_F90), "davp_"), see=as_fortran_sees) == []
    doors = fortran_procedures(read(C_API_F90), "fdp_")
    assert set(doors) == DOORS and mismatches(doors, table_signatures(_abi.PRECOND_FD)) == []
    for table in (_abi.PRECOND, _abi.PRECOND_FD):
        assert not set(table) & (set(_abi.DAV) | set(_abi.FD) | set(_abi.EXT) | set(_abi.EXT_FD) | set(_abi.HERM) | set(_abi.HERM_FD))
    pkg = os.path.join(ROOT, "fortran_davidson_amd")
    called = {name for f in os.listdir(pkg) if f.endswith(".py") for name in re.findall(r"\.((?:davp|fdp)_\w+)\(", read(os.path.join(pkg, f)))}
    assert called == ENTRIES | DOORS


def test_the_abi_stays_109():
    assert re.search(r"#define\s+DAV_HIP_ABI_VERSION\s+109\b", read(os.path.join(ROOT, "include", "davidson_hip.h")))
    assert "DAV_HIP_ABI_VERSION" not in strip_c_comments(read(PRECOND_H))
    assert re.search(r"DAV_KIND_FSAI\s*=\s*10\b", read(os.path.join(ROOT, "fortran_davidson_amd", "csrc", "common.h")))


def test_the_front_ends_exist():
    assert callable(fd.CEngine.build_fsai) and callable(fd.CEngine.fsai_info) and callable(fd.CEngine.fsai_factor)
    assert callable(fd.DavidsonEngine.build_preconditioner)
    engine_f90 = read(os.path.join(ROOT, "fortran_davidson_amd", "fortran", "davidson_engine.f90"))
    assert re.search(r"subroutine engine_build_preconditioner\(eng, sigma, level, stat\)", engine_f90)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def held_to_the_bound(a, b, sigma, level):
    pat = F.pattern(a, level)
    rp, ci, vals, bad = F.fsai_rows(a, b, sigma, level, pat)
    assert bad is None and np.isfinite(vals).all()
    ref, conds = F.reference_rows(a, b, sigma, pat)
    err, bound = F.row_errors(pat, vals, ref), F.row_bounds(pat, ref, conds)
    assert (err <= bound).all(), (int(np.argmax(err / bound)), float((err / bound).max()))
    return pat, conds


@pytest.mark.parametrize("form", ["full", "lower"])
def test_the_restatement_agrees_with_linalg_solve_on_the_banded_matrix(form):
    full, low = F.t1_case(300)
    a = F.canonical(*low, lower=True) if form == "lower" else F.canonical(*full)
    pat, conds = held_to_the_bound(a, None, 0.0, 1)
    assert F.longest_row(pat) == 64 and set(np.diff(pat[0])) == set(range(1, 65))
    assert conds.max() < 6.5


@pytest.mark.parametrize("gev", [False, True])
def test_the_restatement_agrees_with_linalg_solve_on_the_laplacian(gev):
    for shape in ((3, 5), (20, 20)):
        ad, bd = F.level_case(shape, gev)
        a, b = F.dense_csr(ad), None if bd is None else F.dense_csr(bd)
        for level in (1, 2, 3):
            for sigma in (0.0, -1.0):
                pat, conds = held_to_the_bound(a, b, sigma, level)
                assert conds.max() < 6.5
        # G C G^T has a unit diagonal and M = G^T G is symmetric positive definite
        rp, ci, vals, _ = F.fsai_rows(a, b, 0.0, 2)
        g = F.dense_factor(ad.shape[0], rp, ci, vals)
        assert np.allclose(np.diag(g @ ad @ g.T), 1.0, rtol=0, atol=1e-13)
        assert np.linalg.eigvalsh(g.T @ g)[0] > 0.0


def power_of_the_lower_triangle(ad, level):
    """(indptr, indices) of the non-zeros of tril(A)^level, from dense boolean products: independent of fsai_inputs.pattern"""
    low = (np.tril(ad) != 0.0) | np.eye(ad.shape[0], dtype=bool)
    reach = low.copy()
    for _ in range(1, level):
        reach = (reach.astype(np.int64) @ low.astype(np.int64)) > 0
    indptr = np.concatenate([[0], np.cumsum(reach.sum(axis=1))]).astype(np.int64)
    return indptr, np.nonzero(reach)[1].astype(np.int32)


@pytest.mark.parametrize("level", [1, 2, 3])
def test_the_pattern_is_that_of_the_power_of_the_lower_triangle(level):
    """tril(A)^level, not tril(A^level): on the 5-point Laplacian of a 20 x 20 grid 1160 / 2241 / 3605 entries and at most 3 / 6 / 10 per
    row, where tril(A^level) has 1160 / 2602 / 4650 and 3 / 7 / 13 - the column i - nx + 1 of A^2 is reached only through row i + 1"""
    ad = P.solve_case("n400_std")[0]
    pat = F.pattern(F.dense_csr(ad), level)
    want = power_of_the_lower_triangle(ad, level)
    assert np.array_equal(pat[0], want[0]) and np.array_equal(pat[1], want[1])
    assert (pat[1].size, F.longest_row(pat)) == {1: (1160, 3), 2: (2241, 6), 3: (3605, 10)}[level]
    full = np.tril(np.linalg.matrix_power((ad != 0.0).astype(np.int64), level)) > 0
    assert (int(full.sum()), int(full.sum(axis=1).max())) == {1: (1160, 3), 2: (2602, 7), 3: (4650, 13)}[level]
    banded = F.banded(70, 5)
    pb, wb = F.pattern(F.dense_csr(banded), level), power_of_the_lower_triangle(banded, level)
    assert np.array_equal(pb[0], wb[0]) and np.array_equal(pb[1], wb[1])


def test_a_failed_pivot_names_the_smallest_row():
    ad = P.hamiltonian(3, 5, 0.5, 3)[0]
    a = F.dense_csr(ad)
    assert F.fsai_rows(a, None, 0.0, 2)[3] is None
    bad = F.fsai_rows(a, None, 3.2, 2)[3]
    assert bad is not None and bad > 0
    # the first row whose gathered matrix is not positive definite, by its eigenvalues
    pat = F.pattern(a, 2)
    first = next(i for i in range(ad.shape[0])
                 if np.linalg.eigvalsh(F.gathered(a, None, 3.2, pat[1][pat[0][i]:pat[0][i + 1]]))[0] <= 0.0)
    assert bad == first


@pytest.mark.parametrize("name", list(P.SOLVE_CASES))
def test_the_restated_solve_with_the_built_m_needs_at_most_half_the_iterations(name):
    a, b, _, lowest = P.solve_case(name)
    lam0, _, it0 = F.restated_iterations(name)
    assert it0 <= P.MAX_ITERATIONS
    for level in (1, 2, 3):
        lam, x, it = F.restated_iterations(name, level)
        print(f"{name}: plain DPR {it0} iterations, with the restated M of level {level}: {it}")
        assert it <= P.MAX_ITERATIONS and 2 * it <= it0, (level, it, it0)
        assert np.abs(lam - P.eigh_lowest(a, b, lowest)).max() < 1e-9
        assert (P.residual_norms(a, b, lam, x) < P.TOLERANCE).all()


def test_no_input_of_the_gpu_tests_has_a_pattern_row_above_64_except_the_refusal():
    for n in F.T1_SIZES:
        full, low = F.t1_case(n)
        assert F.longest_row(F.pattern(F.canonical(*full), 1)) == min(n, 64)
        assert np.array_equal(F.pattern(F.canonical(*low, lower=True), 1)[1], F.pattern(F.canonical(*full), 1)[1])
    for shape, longest in (((3, 5), (3, 6, 9)), ((20, 20), (3, 6, 10))):          # three grid rows are too few for the tenth column
        for level in (1, 2, 3):
            assert F.longest_row(F.pattern(F.dense_csr(F.level_case(shape, False)[0]), level)) == longest[level - 1]
    for name in P.SOLVE_CASES:
        assert F.longest_row(F.pattern(F.dense_csr(P.solve_case(name)[0]), 3)) == 10
    assert F.longest_row(F.pattern(F.dense_csr(P.hamiltonian(12, 20, 0.5, 5)[0]), 2)) == 6
    refusal = F.pattern(F.dense_csr(F.banded(70, 64)), 1)
    lengths = np.diff(refusal[0])
    assert int(np.argmax(lengths > 64)) == 64 and lengths[64] == 65
    level2 = np.diff(F.pattern(F.dense_csr(F.banded(70, 63)), 2)[0])
    assert int(np.argmax(level2 > 64)) == 64 and level2[64] == 65
