"""The built block preconditioner as a Fortran user sees it (tests/fortran/prog_bfsai.f90): engine_build_block_preconditioner on a
resident engine with a bsr_matrix and with a zcsr_matrix.  The program compiles and links against the modules (CPU) and runs on the GPU
on the multi-orbital pencil (6 x 5 sites, 3 orbitals) and the Peierls lattice of tests/bfsai_inputs.py - both travel in a file - where
its iteration counts equal those of the Python front end, its eigenvalues numpy.linalg.eigh's, and a refused build comes back in stat."""
import os
import re
import subprocess

import numpy as np
import pytest

import fortran_davidson_amd as fd
import bfsai_inputs as BF
import herm_inputs as H
import precond_inputs as P
from test_fortran_programs import FC, MODDIR, SRC, compile_link

needs_flang = pytest.mark.skipif(not os.path.exists(FC), reason="flang not available")
GRID = (6, 5, 3)
LOWEST = 4


def build_bfsai_program(tmp_path):
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    return compile_link([os.path.join(SRC, "prog_bfsai.f90")], os.path.join(bindir, "prog_bfsai"), tmp_path)


@needs_flang
def test_bfsai_program_compiles_and_links(tmp_path):
    if not os.path.isdir(MODDIR):
        pytest.skip("module files not built")
    assert os.path.exists(build_bfsai_program(tmp_path))


@needs_flang
@pytest.mark.gpu
def test_bfsai_program_runs_on_gpu_and_counts_as_the_python_front_end(tmp_path):
    exe = build_bfsai_program(tmp_path)
    ad, _, _, sigma = BF.multi_orbital(*GRID, False)
    rp, ci, blocks = BF.orbital_stores(*GRID, False)[0]
    hm = H.fortran_matrix(12)
    hrp, hci, hval = H.dense_csr(hm)
    path = tmp_path / "matrices.bin"
    with open(path, "wb") as f:
        np.array([rp.size - 1, blocks.shape[1], ci.size], dtype=np.int32).tofile(f)
        (rp + 1).astype(np.int32).tofile(f)
        (ci + 1).astype(np.int32).tofile(f)
        np.ascontiguousarray(blocks.transpose(0, 2, 1)).tofile(f)          # values(r, c, p) in Fortran order
        np.array([sigma], dtype=np.float64).tofile(f)
        np.array([hm.shape[0], hci.size], dtype=np.int32).tofile(f)
        (hrp + 1).astype(np.int32).tofile(f)
        (hci + 1).astype(np.int32).tofile(f)
        np.ascontiguousarray(np.stack([hval.real, hval.imag], axis=1)).tofile(f)
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    out = res.stdout + res.stderr
    assert res.returncode == 0, out
    checks = re.findall(r"CHECK (\S+) ([TF])", out)
    assert len(checks) == 2 + 2 * 2 + 1 + 3 and all(v == "T" for _, v in checks), out
    iters = [int(x) for x in re.search(r"ITERS_BSR\s+(\d+)\s+(\d+)\s+(\d+)", out).groups()]
    info = [int(x) for x in re.search(r"INFO_BSR" + r"\s+(\d+)" * 8, out).groups()]
    herm_iters = [int(x) for x in re.search(r"ITERS_HERM\s+(\d+)\s+(\d+)", out).groups()]
    herm_info = tuple(int(x) for x in re.search(r"INFO_HERM" + r"\s+(\d+)" * 4, out).groups())
    python = []
    with fd.DavidsonEngine(ad.shape[0], LOWEST, None) as eng:
        eng.set_block_sparse(1, rp, ci, blocks)
        python.append((eng.solve("DPR", P.MAX_ITERATIONS, P.TOLERANCE)[2], ()))
        for level in (1, 2):
            built = eng.build_block_preconditioner(sigma, level)
            python.append((eng.solve("DPR", P.MAX_ITERATIONS, P.TOLERANCE)[2], built))
    with fd.DavidsonEngine(2 * hm.shape[0], 2 * LOWEST, None) as eng:
        eng.set_hermitian(1, (hrp, hci, hval))
        herm_python = [eng.solve("DPR", P.MAX_ITERATIONS, P.TOLERANCE)[2]]
        herm_built = eng.build_block_preconditioner()
        herm_python.append(eng.solve("DPR", P.MAX_ITERATIONS, P.TOLERANCE)[2])
    print(f"prog_bfsai: bsr_matrix plain DPR {iters[0]} iterations, built M {iters[1]} (level 1), {iters[2]} (level 2); Python "
          f"{[p[0] for p in python]}; zcsr_matrix {herm_iters}, Python {herm_python}")
    assert iters == [p[0] for p in python]
    assert tuple(info[:4]) == python[1][1] and tuple(info[4:]) == python[2][1]
    assert herm_iters == herm_python and herm_info == herm_built
    ref = np.linalg.eigvalsh(ad)[:LOWEST]
    for label in ("EVALS_PLAIN", "EVALS_LEVEL1", "EVALS_LEVEL2"):
        ev = np.array([float(x) for x in re.search(label + r"(.*)", out).group(1).split()])
        assert np.abs(ev - ref).max() < 1e-8, label
    ev = np.array([float(x) for x in re.search(r"EVALS_HERM(.*)", out).group(1).split()])
    assert np.abs(ev - np.repeat(np.linalg.eigvalsh(hm)[:LOWEST], 2)).max() < 1e-8
