"""The preconditioner slot as a Fortran user sees it (tests/fortran/prog_precond.f90): engine_set_sparse(eng, 3, ...) on a resident
engine and the keyword preconditioner= of the one-shot generic, with a csr_matrix and with a bsr_matrix.  The program compiles and
links against the modules (CPU) and runs on the GPU: every solve with M has the eigenvalues of the plain DPR solve - and of
numpy.linalg.eigh on the matrix rebuilt here from the same integer formula - in fewer iterations."""
import os
import re

import numpy as np
import pytest

import precond_inputs as P
from test_fortran_programs import FC, MODDIR, SRC, _run, compile_link

needs_flang = pytest.mark.skipif(not os.path.exists(FC), reason="flang not available")


def build_precond_program(tmp_path):
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    return compile_link([os.path.join(SRC, "prog_precond.f90")], os.path.join(bindir, "prog_precond"), tmp_path)


def fortran_matrix(nx=16):
    """the matrix tests/fortran/prog_precond.f90 builds, from the same integer formula"""
    n = nx * nx
    p = np.arange(1, n + 1)
    return P.laplacian(nx, nx) + np.diag(0.5 * ((37 * p + 11) % 101) / 101.0)


@needs_flang
def test_precond_program_compiles_and_links(tmp_path):
    if not os.path.isdir(MODDIR):
        pytest.skip("module files not built")
    assert os.path.exists(build_precond_program(tmp_path))


@needs_flang
@pytest.mark.gpu
def test_precond_program_runs_on_gpu(tmp_path):
    exe = build_precond_program(tmp_path)
    rc, out = _run(exe)
    assert rc == 0, out
    it_plain, it_eng, it_csr, it_bsr = [int(x) for x in re.search(r"ITERS\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", out).groups()]
    print(f"prog_precond: plain DPR {it_plain} iterations; with M {it_eng} (engine), {it_csr} (preconditioner= csr), {it_bsr} (bsr)")
    assert max(it_eng, it_csr, it_bsr) < it_plain <= 400
    assert it_eng == it_csr
    ref = np.linalg.eigvalsh(fortran_matrix())[:4]
    for label in ("EVALS_PLAIN", "EVALS_ENGINE", "EVALS_CSR", "EVALS_BSR"):
        ev = np.array([float(x) for x in re.search(label + r"(.*)", out).group(1).split()])
        assert np.abs(ev - ref).max() < 1e-8, label
    checks = re.findall(r"CHECK (\S+) ([TF])", out)
    assert len(checks) == 8 + 3 * 4 and all(v == "T" for _, v in checks), out
