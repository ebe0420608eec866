"""COO triples as a Fortran user sees them (tests/fortran/prog_coo.f90): a coo_matrix through the one-shot generic, through
engine_set_sparse on a resident engine, and engine_update_sparse_values with the values in the order of the triples.  The program
compiles and links against the modules (CPU) and runs on the GPU: every solve prints the digits of the csr_matrix solve of the row
form - the stable sort of the triples by row, which the program does itself."""
import os
import re

import pytest

from test_fortran_programs import FC, MODDIR, SRC, _run, compile_link

needs_flang = pytest.mark.skipif(not os.path.exists(FC), reason="flang not available")


def build_coo_program(tmp_path):
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    return compile_link([os.path.join(SRC, "prog_coo.f90")], os.path.join(bindir, "prog_coo"), tmp_path)


@needs_flang
def test_coo_program_compiles_and_links(tmp_path):
    if not os.path.isdir(MODDIR):
        pytest.skip("module files not built")
    assert os.path.exists(build_coo_program(tmp_path))


@needs_flang
@pytest.mark.gpu
def test_coo_program_prints_the_digits_of_the_row_form(tmp_path):
    rc, out = _run(build_coo_program(tmp_path))
    assert rc == 0, out
    evals = {name: re.search(r"EVALS_" + name + r"\s(.*)", out).group(1).split() for name in ("CSR", "COO", "ENGINE", "UPDATED", "CSR_SCALED")}
    iters = [int(x) for x in re.search(r"ITERS((?:\s+\d+){5})", out).group(1).split()]
    assert all(len(v) == 4 for v in evals.values()), out
    assert evals["COO"] == evals["CSR"] and evals["ENGINE"] == evals["CSR"], out
    assert evals["UPDATED"] == evals["CSR_SCALED"] and evals["UPDATED"] != evals["CSR"], out
    assert iters[1] == iters[0] and iters[2] == iters[0] and iters[3] == iters[4] and 0 < max(iters) < 400, out
