"""CPU: the preconditioner slot (DAV_OP_M) outside the GPU - the constant in every layer, the Python refusals of the entries that serve
A and B only (raised before a door is called: the doors stop the process on an engine error), and the condition on the inputs of the
GPU solve tests: with T = M R the numpy restatement of the solve needs at most half the iterations of plain DPR, so that the same
inequality in tests/test_precond_gpu.py cannot pass trivially."""
import os
import re

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd import engine_c, solver
import precond_inputs as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_slot_has_the_same_number_in_every_layer():
    header = re.search(r"enum\s*\{\s*DAV_OP_A\s*=\s*0\s*,\s*DAV_OP_B\s*=\s*1\s*,\s*DAV_OP_M\s*=\s*(\d+)\s*\}", _text("include", "davidson_hip.h"))
    assert header and int(header.group(1)) == 2
    fortran = re.search(r"integer\(c_int\), parameter :: DAV_OP_M = (\d+)", _text("fortran_davidson_amd", "fortran", "davidson_hip_c.f90"))
    assert fortran and int(fortran.group(1)) == 2
    assert (engine_c.OP_A, engine_c.OP_B, engine_c.OP_M) == (0, 1, 2)
    # DavidsonEngine numbers its slots as the Fortran routines do, from 1
    assert (solver.OP_A, solver.OP_B, solver.OP_M) == (1, 2, 3) and solver.OP_M == engine_c.OP_M + 1


class _NoCalls:
    """a library stand-in whose every symbol fails the test when called (as in tests/test_methods_cpu.py)"""
    def __getattr__(self, name):
        def call(*args):
            raise AssertionError(f"{name} was called")
        return call


class _Engine(fd.DavidsonEngine):
    def __init__(self):
        self.lib, self.c, self.gev, self.n, self.nranks, self.lowest, self.max_dim, self.p = _NoCalls(), _NoCalls(), False, 24, 1, 2, 20, None


REFUSED = {
    "set_dense": lambda e: e.set_dense(3, np.eye(24)),
    "read_matrix": lambda e: e.read_matrix(3, "no_such_file.txt"),
    "generate_diagonal_dominant": lambda e: e.generate_diagonal_dominant(3, 1e-2),
    "set_hashed_operator": lambda e: e.set_hashed_operator(3, 1e-2),
    "set_harness_operator": lambda e: e.set_harness_operator(3),
}


@pytest.mark.parametrize("entry", list(REFUSED))
def test_python_refuses_the_slot_before_any_door_is_called(entry, monkeypatch):
    monkeypatch.setattr(solver, "fortran_lib", lambda: _NoCalls())
    e = _Engine()
    with pytest.raises(ValueError, match="DAV_OP_M") as info:
        REFUSED[entry](e)
    assert entry in str(info.value)
    # ... and the same entries still reach their doors for A and B
    with pytest.raises(AssertionError, match="was called"):
        {"set_dense": lambda: e.set_dense(1, np.eye(24)), "read_matrix": lambda: e.read_matrix(2, "no_such_file.txt"),
         "generate_diagonal_dominant": lambda: e.generate_diagonal_dominant(1, 1e-2), "set_hashed_operator": lambda: e.set_hashed_operator(2, 1e-2),
         "set_harness_operator": lambda: e.set_harness_operator(1)}[entry]()


def test_the_bookkeeping_of_the_engine_holds_three_slots_and_bdpr_reads_two():
    e = _Engine()
    e._note_blocks(1, 4)
    e._note_blocks(3, 16)
    assert e._blocks == [4, None, 16] and e._sparse == [True, False, True]
    # BDPR's checks see A and B only: a preconditioner of another block size is no concern of a method that does not apply it
    with pytest.raises(AssertionError, match="fd_engine_solve was called"):
        e.solve("BDPR")


def test_a_device_operator_goes_without_its_diagonal_only_in_the_slot():
    class Lib(_NoCalls):
        pass
    c = fd.CEngine.__new__(fd.CEngine)
    c.lib, c.h, c.n = Lib(), None, 8
    with pytest.raises(ValueError, match="OP_M"):
        c.set_operator_device(engine_c.OP_A, None, 0, None)
    with pytest.raises(AssertionError, match="dav_set_operator_device was called"):
        c.set_operator_device(engine_c.OP_M, None, 0, None)


@pytest.mark.parametrize("name", list(P.SOLVE_CASES))
def test_the_restated_solve_with_m_needs_at_most_half_the_iterations(name):
    a, b, m, lowest = P.solve_case(name)
    lam0, _, it0 = P.restated_solve(a, lowest, b)
    lam1, x1, it1 = P.restated_solve(a, lowest, b, m)
    print(f"{name}: plain DPR {it0} iterations, T = M R {it1}")
    assert it0 <= P.MAX_ITERATIONS and it1 <= P.MAX_ITERATIONS
    assert 2 * it1 <= it0, (it0, it1)
    ref = P.eigh_lowest(a, b, lowest)
    assert np.abs(lam1 - ref).max() < 1e-9 and np.abs(lam0 - ref).max() < 1e-9
    assert (P.residual_norms(a, b, lam1, x1) < P.TOLERANCE).all()


def test_the_builders_of_m_restate_the_same_matrix():
    a = P.int_banded(48, 3)
    assert np.array_equal(a, a.T)
    rp, ci, vv = P.csr_of(a)
    dense = np.zeros_like(a)
    dense[np.repeat(np.arange(48), np.diff(rp)), ci] = vv
    assert np.array_equal(dense, a)
    for b in (3, 16):
        rp, ci, vv = P.bsr_of(a, b)
        dense = np.zeros_like(a)
        for i in range(48 // b):
            for p in range(rp[i], rp[i + 1]):
                dense[i * b:(i + 1) * b, ci[p] * b:(ci[p] + 1) * b] = vv[p]
        assert np.array_equal(dense, a)
    full = P.csr_of(np.eye(5), full=True)
    assert full[0][-1] == 25 and full[2].size == 25
    bm = P.mass_matrix(400, 112)
    off = np.abs(bm - np.diag(np.diag(bm))).sum(axis=1)
    assert np.array_equal(bm, bm.T) and (off < 1.0).all() and (np.diag(bm) == 1.0).all()
