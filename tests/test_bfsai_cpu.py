"""CPU: the block preconditioner the engine builds from BSR and Hermitian operators (davq_build_block_fsai) exists in every layer.  Its
entries are extension entries next to ABI 109 (include/davidson_hip_bprecond.h, prefix davq_; doors prefix fdq_): both builds of the engine
export exactly the three entries and the Fortran library the two doors; the four mirrors - header, ctypes tables, Fortran interface
module, doors - are compared the way tests/test_fsai_cpu.py compares its own; the ABI stays 109.  The numpy restatement of the block row
(tests/bfsai_inputs.py) agrees with numpy.linalg.solve scalar row by scalar row within the bound the GPU tests use, equals the scalar
restatement of the expanded matrix within the sum of the two bounds, gives (G C G^T)_II = I_b and, on the Peierls lattice, blocks of the
form [[x, -y], [y, x]]; the restated solves meet the inequalities the GPU solves are held to, and no input of the GPU tests has a block
row of more than 64 scalar columns except the one made for the refusal."""
import os
import re
import subprocess

import numpy as np
import pytest

import fortran_davidson_amd as fd
import bfsai_inputs as BF
import fsai_inputs as F
import precond_inputs as P
from fortran_davidson_amd import _abi
from test_abi_cpu import C_API_F90, HIP_C_F90, as_fortran_sees, c_class, fortran_procedures, mismatches, read, strip_c_comments, table_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fortran_davidson_amd", "lib")
BPRECOND_H = os.path.join(ROOT, "include", "davidson_hip_bprecond.h")
ENTRIES = {"davq_build_block_fsai", "davq_block_fsai_info", "davq_block_fsai_get_factor"}
DOORS = {"fdq_engine_build_block_fsai", "fdq_engine_block_fsai_info"}


def exported(lib, prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return set(re.findall(rf"\s[TW]\s+({prefix}\w+)$", out, re.M))


def bprecond_prototypes():
    return {name: ("i32", tuple(c_class(a.strip()) for a in args.split(",")))
            for name, args in re.findall(r"\bint\s+(davq_\w+)\s*\(([^()]*)\)\s*;", strip_c_comments(read(BPRECOND_H)))}


def test_both_libraries_export_the_entries_and_the_doors():
    for lib in (os.path.join(LIBDIR, "libdavidson_hip.so"), os.path.join(LIBDIR, "test", "libdavidson_hip.so")):
        assert exported(lib, "davq_") == ENTRIES, lib
    assert exported(os.path.join(LIBDIR, "libfortran_davidson_amd.so"), "fdq_") == DOORS
    syms = subprocess.run(["strings", os.path.join(LIBDIR, "libdavidson_hip.so")], capture_output=True, text=True, check=True).stdout
    assert "bfsai_rows_kernel" in syms


def test_the_four_mirrors_are_equal():
    header = bprecond_prototypes()
    assert set(header) == ENTRIES
    assert header["davq_build_block_fsai"] == ("i32", ("ptr", "f64", "i32"))
    assert header["davq_block_fsai_info"] == ("i32", ("ptr", "ptr", "ptr", "ptr", "ptr"))
    assert header["davq_block_fsai_get_factor"] == ("i32", ("ptr", "i32", "ptr", "ptr", "ptr"))
    assert mismatches(header, table_signatures(_abi.BPRECOND)) == []
    assert mismatches(header, fortran_procedures(read(HIP_C_F90), "davq_"), see=as_fortran_sees) == []
    doors = fortran_procedures(read(C_API_F90), "fdq_")
    assert set(doors) == DOORS and mismatches(doors, table_signatures(_abi.BPRECOND_FD)) == []
    others = (_abi.DAV, _abi.FD, _abi.EXT, _abi.EXT_FD, _abi.HERM, _abi.HERM_FD, _abi.PRECOND, _abi.PRECOND_FD)
    for table in (_abi.BPRECOND, _abi.BPRECOND_FD):
        assert not set(table) & set().union(*(set(t) for t in others))
    pkg = os.path.join(ROOT, "fortran_davidson_amd")
    called = {name for f in os.listdir(pkg) if f.endswith(".py") for name in re.findall(r"\.((?:davq|fdq)_\w+)\(", read(os.path.join(pkg, f)))}
    assert called == ENTRIES | DOORS


def test_the_abi_stays_109():
    assert re.search(r"#define\s+DAV_HIP_ABI_VERSION\s+109\b", read(os.path.join(ROOT, "include", "davidson_hip.h")))
    assert "DAV_HIP_ABI_VERSION" not in strip_c_comments(read(BPRECOND_H))
    common = read(os.path.join(ROOT, "fortran_davidson_amd", "csrc", "common.h"))
    assert re.search(r"DAV_KIND_BFSAI\s*=\s*11\b", common) and re.search(r"DAV_KIND_FSAI\s*=\s*10\b", common)


def test_the_front_ends_exist():
    assert callable(fd.CEngine.build_block_fsai) and callable(fd.CEngine.block_fsai_info) and callable(fd.CEngine.block_fsai_factor)
    assert callable(fd.DavidsonEngine.build_block_preconditioner)
    fortran = os.path.join(ROOT, "fortran_davidson_amd", "fortran")
    engine_f90 = read(os.path.join(fortran, "davidson_engine.f90"))
    assert re.search(r"subroutine engine_build_block_preconditioner\(eng, sigma, level, stat\)", engine_f90)
    assert re.search(r"subroutine engine_block_preconditioner_info\(", engine_f90)
    assert re.search(r"engine_build_block_preconditioner, engine_block_preconditioner_info", read(os.path.join(fortran, "davidson.f90")))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def held_to_the_bound(a, bm, sigma, level, tag):
    """the restated block rows within the bound of the reference, and within the sum of the two bounds of the scalar restatement of the
    expanded matrix; returns (block pattern, blocks, conds)"""
    b = a[2].shape[1]
    bpat = BF.block_pattern(a, level)
    rp, ci, blocks, bad = BF.bfsai_rows(a, bm, sigma, level, bpat)
    assert bad is None and np.isfinite(blocks).all(), tag
    spat, ref, conds = BF.reference(a, bm, sigma, bpat)
    vals = BF.scalar_rows(bpat, b, blocks)
    err, bound = F.row_errors(spat, vals, ref), F.row_bounds(spat, ref, conds)
    assert (err <= bound).all(), (tag, int(np.argmax(err / bound)), float((err / bound).max()))
    # the scalar pattern of the expanded matrix is the lower triangle of the block pattern, and its restated rows are the same G
    ea, eb = BF.expanded_of(a), None if bm is None else BF.expanded_of(bm)
    epat = F.pattern(ea, level)
    assert np.array_equal(epat[0], spat[0]) and np.array_equal(epat[1], spat[1]), tag
    scalar = F.fsai_rows(ea, eb, sigma, level, spat)[2]
    assert (F.row_errors(spat, vals, scalar) <= 2.0 * bound).all(), tag
    # above the diagonal of the diagonal blocks: +0.0
    diag = blocks[rp[1:] - 1]
    upper = diag[:, np.triu_indices(b, 1)[0], np.triu_indices(b, 1)[1]]
    assert not upper.any() and not np.signbit(upper).any(), tag
    return bpat, blocks, conds


@pytest.mark.parametrize("b", BF.BLOCK_SIZES)
def test_the_restatement_agrees_with_linalg_solve_on_the_block_banded_matrix(b):
    cap = (BF.MAX_COLS // b) * b
    for nb in BF.banded_sizes(b):
        full, low = BF.banded_case(b, nb)
        for form, a in (("full", BF.canonical_blocks(*full)), ("lower", BF.canonical_blocks(*low, lower=True))):
            bpat, blocks, conds = held_to_the_bound(a, None, 0.0, 1, f"banded b={b} nb={nb} {form}")
            s = np.diff(bpat[0]) * b
            assert s.max() == min(nb * b, cap)
            if nb == BF.banded_sizes(b)[-1]:          # every s from b to the cap, and both instances of the kernel
                assert set(s) == set(range(b, cap + 1, b)), (b, nb)
                assert (s <= 16).any() and (s > 16).any()
            assert conds.max() < 8.0, conds.max()
        assert low[1].size > np.unique(np.stack([np.repeat(np.arange(nb), np.diff(low[0])), low[1]]), axis=1).shape[1] or nb == 1
        n = nb * b
        assert np.allclose(BF.dense_of(BF.canonical_blocks(*low, lower=True), n), BF.dense_of(BF.canonical_blocks(*full), n), rtol=0, atol=1e-13)


@pytest.mark.parametrize("gev", [False, True])
def test_the_restatement_agrees_with_linalg_solve_on_the_multi_orbital_pencil(gev):
    nx, ny, b = 6, 5, 3
    ad, bd, _, sigma0 = BF.multi_orbital(nx, ny, b, gev)
    sa, sb = BF.orbital_stores(nx, ny, b, gev)
    a, bm = BF.canonical_blocks(*sa), None if sb is None else BF.canonical_blocks(*sb)
    assert np.array_equal(BF.dense_of(a, ad.shape[0]), ad)
    worst = 0.0
    for level in (1, 2, 3):
        for sigma in (0.0, -1.0, sigma0):
            bpat, blocks, conds = held_to_the_bound(a, bm, sigma, level, f"orbital gev={gev} level={level} sigma={sigma}")
            worst = max(worst, conds.max())
            # (G C G^T)_II = I_b and M = G^T G is positive definite
            g = BF.dense_factor(ad.shape[0], bpat[0], bpat[1], blocks)
            c = ad - sigma * (np.eye(ad.shape[0]) if bd is None else bd)
            gcg = g @ c @ g.T
            for i in range(nx * ny):
                assert np.allclose(gcg[i * b:(i + 1) * b, i * b:(i + 1) * b], np.eye(b), rtol=0, atol=1e-13)
            assert np.linalg.eigvalsh(g.T @ g)[0] > 0.0
    print(f"multi-orbital gev={gev}: largest cond_2 {worst:.3g}")
    assert worst < 16.0, worst


@pytest.mark.parametrize("gev", [False, True])
def test_the_peierls_factor_is_the_real_form_of_a_complex_one(gev):
    sa, sb = BF.peierls_stores(gev)
    a, bm = BF.canonical_blocks(*sa), None if sb is None else BF.canonical_blocks(*sb)
    c = BF.solve_case("peierls_gev" if gev else "peierls_std")
    worst = 0.0
    for level in (1, 2, 3):
        bpat, blocks, conds = held_to_the_bound(a, bm, 0.0, level, f"peierls gev={gev} level={level}")
        worst = max(worst, conds.max())
        # every 2 x 2 block of G is [[x, -y], [y, x]]: M is the real form of a Hermitian matrix and keeps every eigenvalue paired
        scale = np.abs(blocks).max()
        off = max(np.abs(blocks[:, 0, 0] - blocks[:, 1, 1]).max(), np.abs(blocks[:, 0, 1] + blocks[:, 1, 0]).max())
        print(f"peierls gev={gev} level {level}: deviation from [[x, -y], [y, x]] {off / scale:.3g} of the largest entry")
        assert off <= 1e-14 * scale
        g = BF.dense_factor(c["a"].shape[0], bpat[0], bpat[1], blocks)
        gcg = g @ c["a"] @ g.T          # sigma = 0
        assert np.allclose(gcg[np.arange(gcg.shape[0]), np.arange(gcg.shape[0])], 1.0, rtol=0, atol=1e-13)
        assert np.abs(gcg[0::2, 1::2].diagonal()).max() < 1e-13
        assert np.linalg.eigvalsh(g.T @ g)[0] > 0.0
    print(f"peierls gev={gev}: largest cond_2 {worst:.3g}")
    assert worst < 8.0, worst


def test_a_failed_pivot_names_the_smallest_block_row():
    nx, ny, b = 6, 5, 3
    ad, _, _, sigma0 = BF.multi_orbital(nx, ny, b, False)
    a = BF.canonical_blocks(*BF.orbital_stores(nx, ny, b, False)[0])
    assert BF.bfsai_rows(a, None, sigma0, 2)[3] is None
    sigma = sigma0 + 3.5
    bad = BF.bfsai_rows(a, None, sigma, 2)[3]
    assert bad is not None and bad > 0
    bpat = BF.block_pattern(a, 2)
    cols = lambda i: (bpat[1][bpat[0][i]:bpat[0][i + 1]].astype(np.int64)[:, None] * b + np.arange(b)[None, :]).ravel()          # noqa: E731
    first = next(i for i in range(nx * ny) if np.linalg.eigvalsh(F.gathered(BF.expanded_of(a), None, sigma, cols(i)))[0] <= 0.0)
    assert bad == first


@pytest.mark.parametrize("name", BF.SOLVE_CASES)
def test_the_restated_solves_meet_what_the_gpu_solves_are_held_to(name):
    c = BF.solve_case(name)
    lam0, _, it0 = BF.restated_iterations(name)
    assert it0 <= P.MAX_ITERATIONS
    for level in (1, 2, 3):
        lam, x, it = BF.restated_iterations(name, level)
        print(f"{name}: plain DPR {it0} iterations, with the restated block M of level {level}: {it}")
        assert it <= P.MAX_ITERATIONS
        if name.startswith("orbital") or level >= 2:
            assert 2 * it <= it0, (level, it, it0)
        else:          # level 1 on the Peierls lattice: too close to half for the slack of the GPU test
            assert it < it0, (level, it, it0)
        assert np.abs(lam - P.eigh_lowest(c["a"], c["b"], c["lowest"])).max() < 1e-9
        assert (P.residual_norms(c["a"], c["b"], lam, x) < P.TOLERANCE).all()


def test_no_input_of_the_gpu_tests_has_a_block_row_above_64_columns_except_the_refusal():
    for b in BF.BLOCK_SIZES:
        for nb in BF.banded_sizes(b):
            full, low = BF.banded_case(b, nb)
            pf, pl = BF.block_pattern(BF.canonical_blocks(*full), 1), BF.block_pattern(BF.canonical_blocks(*low, lower=True), 1)
            assert F.longest_row(pf) * b == min(nb, BF.MAX_COLS // b) * b <= BF.MAX_COLS
            assert np.array_equal(pf[1], pl[1])
        refusal = np.diff(BF.block_pattern(BF.canonical_blocks(*BF.banded_refusal(b)), 1)[0])
        first = int(np.argmax(refusal * b > BF.MAX_COLS))
        assert first == 64 // b and refusal[first] == 64 // b + 1 and (refusal[:first] * b <= BF.MAX_COLS).all()
    for gev in (False, True):
        a = BF.canonical_blocks(*BF.orbital_stores(6, 5, 3, gev)[0])
        assert [F.longest_row(BF.block_pattern(a, level)) for level in (1, 2, 3)] == [3, 6, 10]
        nx, ny, b = BF.ORBITAL_SOLVE
        assert F.longest_row(BF.block_pattern(BF.canonical_blocks(*BF.orbital_stores(nx, ny, b, gev)[0]), 3)) * b == 40
        assert F.longest_row(BF.block_pattern(BF.canonical_blocks(*BF.peierls_stores(gev)[0]), 3)) * 2 == 20
    arrow = BF.canonical_blocks(*BF.arrow(), lower=True)
    assert F.longest_row(BF.block_pattern(arrow, 1)) == 2
    # level 2 of a 5-point stencil at b = 16 does not fit: 6 blocks, 96 columns
    assert F.longest_row(BF.block_pattern(BF.canonical_blocks(*BF.orbital_stores(6, 5, 3, False)[0]), 2)) * 16 > BF.MAX_COLS
