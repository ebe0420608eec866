"""The built preconditioner as a Fortran user sees it (tests/fortran/prog_fsai.f90): engine_build_preconditioner on a resident engine.
The program compiles and links against the modules (CPU) and runs on the GPU on the case n400_std of tests/precond_inputs.py - the
potential travels in a file - where its iteration counts equal those of the Python front end and its eigenvalues numpy.linalg.eigh's."""
import os
import re
import subprocess

import numpy as np
import pytest

import fortran_davidson_amd as fd
import precond_inputs as P
from test_fortran_programs import FC, MODDIR, SRC, compile_link

needs_flang = pytest.mark.skipif(not os.path.exists(FC), reason="flang not available")


def build_fsai_program(tmp_path):
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    return compile_link([os.path.join(SRC, "prog_fsai.f90")], os.path.join(bindir, "prog_fsai"), tmp_path)


@needs_flang
def test_fsai_program_compiles_and_links(tmp_path):
    if not os.path.isdir(MODDIR):
        pytest.skip("module files not built")
    assert os.path.exists(build_fsai_program(tmp_path))


@needs_flang
@pytest.mark.gpu
def test_fsai_program_runs_on_gpu_and_counts_as_the_python_front_end(tmp_path):
    exe = build_fsai_program(tmp_path)
    nx, ny, scale, seed, lowest, _ = P.SOLVE_CASES["n400_std"]
    a, _, _, _ = P.solve_case("n400_std")
    potential = tmp_path / "potential.f64"
    P.potential(nx * ny, scale, seed).astype(np.float64).tofile(potential)
    res = subprocess.run([exe, str(potential)], capture_output=True, text=True, timeout=300)
    out = res.stdout + res.stderr
    assert res.returncode == 0, out
    checks = re.findall(r"CHECK (\S+) ([TF])", out)
    assert len(checks) == 2 + 2 * (2 + lowest) and all(v == "T" for _, v in checks), out
    it_plain, it1, it2 = [int(x) for x in re.search(r"ITERS\s+(\d+)\s+(\d+)\s+(\d+)", out).groups()]
    info = [int(x) for x in re.search(r"INFO" + r"\s+(\d+)" * 6, out).groups()]
    python = []
    with fd.DavidsonEngine(a.shape[0], lowest, None) as eng:
        eng.set_sparse(1, *P.csr_of(a))
        python.append((eng.solve("DPR", P.MAX_ITERATIONS, P.TOLERANCE)[2], ()))
        for level in (1, 2):
            built = eng.build_preconditioner(0.0, level)
            python.append((eng.solve("DPR", P.MAX_ITERATIONS, P.TOLERANCE)[2], built))
    print(f"prog_fsai: plain DPR {it_plain} iterations, built M {it1} (level 1), {it2} (level 2); Python {[p[0] for p in python]}")
    assert [it_plain, it1, it2] == [p[0] for p in python]
    assert tuple(info[:3]) == python[1][1] and tuple(info[3:]) == python[2][1]
    ref = np.linalg.eigvalsh(a)[:lowest]
    for label in ("EVALS_PLAIN", "EVALS_LEVEL1", "EVALS_LEVEL2"):
        ev = np.array([float(x) for x in re.search(label + r"(.*)", out).group(1).split()])
        assert np.abs(ev - ref).max() < 1e-8, label
