"""Complex Hermitian operators as a Fortran user sees them (tests/fortran/prog_herm.f90).  On the CPU the program compiles and links
against the modules and its file mode runs hermitian_eigenpairs - host-only code - on numpy real-form pairs, held to the assertions of
tests/test_herm_cpu.py.  On the GPU it solves a Peierls lattice through the zcsr_matrix specific of the generic (a standard problem and a
pencil), through engine_set_hermitian on a resident engine with hermitian_eigenpairs, and after engine_update_hermitian_values; the
eigenvalues are compared with scipy.linalg.eigh on the matrices rebuilt here from the same integer formulas."""
import os
import re
import subprocess

import numpy as np
import pytest

import herm_inputs as H
from test_fortran_programs import FC, MODDIR, SRC, _run, compile_link

needs_flang = pytest.mark.skipif(not os.path.exists(FC), reason="flang not available")


def build_herm_program(tmp_path):
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    return compile_link([os.path.join(SRC, "prog_herm.f90")], os.path.join(bindir, "prog_herm"), tmp_path)


@needs_flang
def test_herm_program_compiles_and_links(tmp_path):
    if not os.path.isdir(MODDIR):
        pytest.skip("module files not built")
    assert os.path.exists(build_herm_program(tmp_path))


@needs_flang
@pytest.mark.parametrize("case", ["generic", "pencil", "cluster_cut"])
def test_fortran_extraction_on_numpy_pairs(case, tmp_path):
    if not os.path.isdir(MODDIR):
        pytest.skip("module files not built")
    sl = pytest.importorskip("scipy.linalg")
    exe = build_herm_program(tmp_path)
    n, lowest = 40, 4
    h, s = H.extraction_case(case, n, lowest)
    a, b = H.real_form(h), None if s is None else H.real_form(s)
    theta, v = sl.eigh(a, b)
    theta, v = theta[:2 * lowest], v[:, :2 * lowest]
    ref = sl.eigh(h, s, eigvals_only=True)
    path = os.path.join(tmp_path, "pairs.txt")
    with open(path, "w") as f:
        f.write(f"{n} {lowest} {int(s is not None)}\n")
        f.write("\n".join(repr(float(t)) for t in theta) + "\n")
        f.write("\n".join(repr(float(t)) for t in v.T.reshape(-1)) + "\n")
        if s is not None:
            rp, ci, vv = H.dense_csr(s)
            f.write(f"{vv.size}\n" + "\n".join(str(int(t) + 1) for t in rp) + "\n" + "\n".join(str(int(t) + 1) for t in ci) + "\n")
            f.write("\n".join(f"{float(z.real)!r} {float(z.imag)!r}" for z in vv) + "\n")
    res = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lam = np.array([float(t) for t in re.search(r"LAMBDA(.*)", res.stdout).group(1).split()])
    xs = np.array([[float(t) for t in m] for m in re.findall(r"^\s*X\s+(\S+)\s+(\S+)", res.stdout, re.M)])
    x = (xs[:, 0] + 1j * xs[:, 1]).reshape(lowest, n).T
    H.check_extraction(h, s, theta, v, lam, x, ref)


def write_zcsr(f, m):
    """one matrix of the program's "solve" file: nnz, row_ptr and col_idx from 1, the (re, im) values"""
    rp, ci, vv = m
    f.write(f"{vv.size}\n" + "\n".join(str(int(t) + 1) for t in rp) + "\n" + "\n".join(str(int(t) + 1) for t in ci) + "\n")
    f.write("\n".join(f"{float(z.real)!r} {float(z.imag)!r}" for z in vv) + "\n")


@needs_flang
@pytest.mark.gpu
def test_herm_program_runs_on_gpu(tmp_path):
    sl = pytest.importorskip("scipy.linalg")
    rc, out = _run(build_herm_program(tmp_path))
    assert rc == 0, out
    h, s = H.fortran_matrix(), H.fortran_overlap()
    ref = {"ONESHOT": sl.eigh(h, eigvals_only=True)[:4], "PENCIL": sl.eigh(h, s, eigvals_only=True)[:4]}
    ref["ENGINE"] = ref["ONESHOT"]
    ref["UPDATED"] = ref["SCALED"] = 1.5 * ref["ONESHOT"]
    for name, want in ref.items():
        ev = np.array([float(t) for t in re.search(r"EVALS_" + name + r"\s(.*)", out).group(1).split()])
        print(name, np.abs(ev - want).max())
        assert np.abs(ev - want).max() <= 1e-8, (name, ev, want)
    iters = [int(t) for t in re.search(r"ITERS((?:\s+\d+){5})", out).group(1).split()]
    assert 0 < max(iters) < 400, out


@needs_flang
@pytest.mark.gpu
@pytest.mark.parametrize("method", ["DPR", "GJD"])
@pytest.mark.parametrize("name", ["graded", "pencil", "double", "lattice"])
def test_the_four_solve_inputs_through_the_fortran_program(name, method, tmp_path):
    """the inputs of the solves of tests/test_herm_gpu.py through engine_set_hermitian with hermitian_eigenpairs and through the
    zcsr_matrix specific: eigenvalues against eigh to 1e-8, and the extraction's assertions on the engine's real-form pairs"""
    sl = pytest.importorskip("scipy.linalg")
    exe = build_herm_program(tmp_path)
    lowest = 4
    h, s = H.solve_matrix(name)
    n = h.shape[0]
    path = os.path.join(tmp_path, "matrix.txt")
    with open(path, "w") as f:
        f.write(f"{n} {lowest} {int(s is not None)} {method}\n")
        write_zcsr(f, H.dense_csr(h))
        if s is not None:
            write_zcsr(f, H.dense_csr(s))
    res = subprocess.run([exe, "solve", path], capture_output=True, text=True, timeout=300)
    out = res.stdout
    assert res.returncode == 0, out[-2000:] + res.stderr
    numbers = lambda pat: np.array([float(t) for t in re.search(pat, out).group(1).split()])          # noqa: E731

    def columns(tag, rows, cols):
        xs = np.array([[float(t) for t in m] for m in re.findall(rf"^\s*{tag}\s+(\S+)\s+(\S+)", out, re.M)])
        return (xs[:, 0] + 1j * xs[:, 1]).reshape(cols, rows).T
    iters = [int(t) for t in re.search(r"ITERS\s+(\d+)\s+(\d+)", out).groups()]
    theta, lam, lam1 = numbers(r"THETA(.*)"), numbers(r"LAMBDA\s(.*)"), numbers(r"LAMBDA1(.*)")
    v = np.array([float(t) for t in re.findall(r"^\s*V\s+(\S+)\s*$", out, re.M)]).reshape(2 * lowest, 2 * n).T
    x, x1 = columns("X", n, lowest), columns("X1", n, lowest)
    ref = sl.eigh(h, s, eigvals_only=True)
    print(f"{name} {method}: {iters} iterations")
    assert 0 < max(iters) < 400 and iters[0] == iters[1]
    assert np.abs(lam - ref[:lowest]).max() <= 1e-8 and np.abs(lam1 - ref[:lowest]).max() <= 1e-8, (lam, lam1, ref[:lowest])
    H.check_extraction(h, s, theta, v, lam, x, ref, tol_lambda=1e-8)
    H.check_extraction(h, s, theta, v, lam1, x1, ref, tol_lambda=1e-8)          # the specific ran the same solve
