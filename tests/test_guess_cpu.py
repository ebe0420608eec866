"""CPU: warm starts without a GPU - the engine entries and the Fortran doors are exported by both libraries, declared in the header and
bound in Fortran; a Fortran program that uses initial_vectors= and the three engine routines next to a positional call with the
reference's argument list compiles and links; the Python front ends check dtype and shape before any engine call."""
import os
import subprocess

import numpy as np
import pytest
import torch

import fortran_davidson_amd as fd
from fortran_davidson_amd.engine_c import CEngine, guess_array
from fortran_davidson_amd import solver
from test_fortran_programs import FC, LIBDIR, MODDIR, SRC, compile_link

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dav_set_guess", "dav_set_guess_dev", "dav_keep_result_as_guess", "dav_mark_result_as_guess", "dav_guess_columns",
           "dav_init_basis_guess")
DOORS = ("fd_engine_set_initial_vectors", "fd_engine_set_initial_vectors_device", "fd_engine_keep_result_as_guess",
         "fd_dense_solve_guess", "fd_sparse_solve_guess", "fd_bsr_solve_guess", "fd_free_solve_guess")


def build_guess_program(workdir):
    bindir = os.path.join(SRC, "_bin")
    os.makedirs(bindir, exist_ok=True)
    return compile_link([os.path.join(SRC, "prog_guess.f90")], os.path.join(bindir, "prog_guess"), workdir)


def test_the_entries_and_the_fortran_doors_are_exported():
    product = os.path.join(LIBDIR, "libdavidson_hip.so")
    names = subprocess.run(["nm", "-D", "--defined-only", product], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "davidson_hip.h")).read()
    f90 = open(os.path.join(ROOT, "fortran_davidson_amd", "fortran", "davidson_hip_c.f90")).read()
    for name in ENTRIES:
        assert hasattr(fd.hip_lib(), name), name            # the library pytest loads (the test build)
        assert f" T {name}\n" in names, name                # the product
        assert f"int {name}(" in hdr
        assert f'bind(C, name="{name}")' in f90
    for name in DOORS:
        assert hasattr(fd.fortran_lib(), name), name
    for method in ("set_guess", "keep_result_as_guess", "guess_columns", "init_basis_guess"):
        assert callable(getattr(CEngine, method))
    for method in ("set_initial_vectors", "keep_result_as_guess"):
        assert callable(getattr(fd.DavidsonEngine, method))


@pytest.mark.skipif(not os.path.exists(FC), reason="flang not available")
def test_guess_program_with_keyword_and_positional_calls_compiles_and_links(tmp_path):
    if not os.path.isdir(MODDIR):
        pytest.skip("module files not built")
    assert os.path.exists(build_guess_program(tmp_path))


class _NoCalls:
    """a library stand-in whose every symbol fails the test when called"""
    def __getattr__(self, name):
        def call(*args):
            raise AssertionError(f"{name} was called")
        return call


def _engine(n):
    e = CEngine.__new__(CEngine)
    e.lib, e.h, e.n, e.device, e.owned = _NoCalls(), None, n, 0, False
    return e


def _front_end(n, lowest):
    eng = fd.DavidsonEngine.__new__(fd.DavidsonEngine)
    eng.n, eng.lowest, eng.max_dim, eng.lib, eng.p, eng.device = n, lowest, 10 * lowest, _NoCalls(), None, 0
    return eng


@pytest.mark.parametrize("bad", [np.float32, np.int64, np.complex128])
def test_numpy_dtypes_are_refused_before_any_call(bad):
    with pytest.raises(TypeError, match="expected float64"):
        _engine(6).set_guess(np.ones((6, 2), dtype=bad))
    with pytest.raises(TypeError, match="expected float64"):
        _front_end(6, 2).solve(initial_vectors=np.ones((6, 2), dtype=bad))


@pytest.mark.parametrize("bad", [torch.float32, torch.int64])
def test_torch_dtypes_are_refused_before_any_call(bad):
    with pytest.raises(TypeError, match="expected torch.float64"):
        _engine(6).set_guess(torch.ones((6, 2), dtype=bad))
    with pytest.raises(TypeError, match="expected torch.float64"):
        _front_end(6, 2).set_initial_vectors(torch.ones((6, 2), dtype=bad))


def test_a_wrong_row_count_is_refused_before_any_call():
    for x in (np.ones((5, 2)), np.ones((7, 1)), np.ones(5), np.ones((6, 2, 1)), np.ones((6, 0)), torch.ones((5, 2), dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"must have shape \(6, ncols\)"):
            _engine(6).set_guess(x)
        with pytest.raises(ValueError, match=r"must have shape \(6, ncols\)"):
            _front_end(6, 2).set_initial_vectors(x)


def test_one_call_front_ends_check_the_guess_before_the_fortran_doors(monkeypatch):
    """their doors stop the process on a refused guess: dtype, rows, finite entries and zero columns are checked in Python"""
    monkeypatch.setattr(solver, "fortran_lib", lambda: _NoCalls())
    a = np.diag(np.arange(1.0, 7.0))
    good = np.eye(6)[:, :2]
    for x, exc, msg in ((good.astype(np.float32), TypeError, "expected float64"), (np.ones((5, 2)), ValueError, "must have shape"),
                        (np.where(np.eye(6)[:, :2] > 0, np.nan, 0.0), ValueError, "not finite"),
                        (np.where(np.eye(6)[:, :2] > 0, np.inf, 0.0), ValueError, "not finite"),
                        (np.column_stack([good[:, 0], -0.0 * good[:, 1]]), ValueError, "column 1 of x")):
        with pytest.raises(exc, match=msg):
            fd.generalized_eigensolver(a, 1, "DPR", 10, 1e-8, initial_vectors=x)
        rp, ci, vv = np.arange(7, dtype=np.int64), np.arange(6, dtype=np.int32), np.arange(1.0, 7.0)
        with pytest.raises(exc, match=msg):
            fd.generalized_eigensolver_sparse(rp, ci, vv, 1, "DPR", 10, 1e-8, initial_vectors=x)
        with pytest.raises(exc, match=msg):
            fd.generalized_eigensolver_bsr(rp, ci, vv.reshape(6, 1, 1), 1, "DPR", 10, 1e-8, initial_vectors=x)


def test_host_data_reaches_the_host_entry_column_major_and_wide_guesses_are_cut():
    seen = {}

    class Lib(_NoCalls):
        def dav_set_guess(self, h, x, ldx, ncols):
            seen["c"] = (ldx, ncols, np.ctypeslib.as_array(x, shape=(ncols, ldx)).T.copy())
            return 0

        def fd_engine_set_initial_vectors(self, p, x, ncols):
            seen["f"] = (ncols, np.ctypeslib.as_array(x, shape=(ncols, 6)).T.copy())
            return 0

    x = np.arange(30.0).reshape(6, 5)                        # C order: the front ends make it column-major
    e = _engine(6)
    e.lib = Lib()
    e.set_guess(x)
    e.set_guess(torch.from_numpy(x))                         # a CPU tensor is host data
    assert seen["c"][:2] == (6, 5) and np.array_equal(seen["c"][2], x)
    host, dev = guess_array(x[:, 0], 6)
    assert dev is None and host.shape == (6, 1)
    eng = _front_end(6, 2)
    eng.lib = Lib()
    eng.set_initial_vectors(x)                               # 5 columns, start basis 2 * lowest = 4: the leading 4 are used
    assert seen["f"][0] == 4 and np.array_equal(seen["f"][1], x[:, :4])


def test_the_reference_list_specifics_keep_their_argument_lists():
    """initial_vectors= selects specifics of its own (_guess): a dummy appended to an existing specific would change its binary interface,
    and a program built against earlier modules would pass it one argument too few (present() then reads what lies there)"""
    src = open(os.path.join(ROOT, "fortran_davidson_amd", "fortran", "davidson.f90")).read()
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libfortran_davidson_amd.so")], capture_output=True, text=True,
                           check=True).stdout.lower()
    for kind in ("dense", "free", "device", "sparse", "bsr"):
        head = src.split(f"subroutine generalized_eigensolver_{kind}(", 1)[1].split(")", 1)[0]
        assert "initial_vectors" not in head, kind
        guess = src.split(f"subroutine generalized_eigensolver_{kind}_guess(", 1)[1].split(")", 1)[0]
        assert guess.replace(" ", "").replace("&\n", "") == head.replace(" ", "").replace("&\n", "") + ",initial_vectors", kind
        assert f"generalized_eigensolver_{kind}\n" in names and f"generalized_eigensolver_{kind}_guess\n" in names
