"""CPU: the COO entries exist in every layer.  They are EXTENSION entries next to ABI 109 (include/davidson_hip_ext.h, prefix davx_; doors
prefix fdx_): the table of dav_* entries that tests/test_abi_cpu.py and the export tests pin entry for entry stays as it is.  Both builds
of the engine export davx_set_operator_coo(_dev) and the Fortran library its doors, the header stays at ABI 109, the four mirrors of the
extension entries - header, ctypes tables, Fortran interface module, doors - are compared the way tests/test_abi_cpu.py compares the
pinned ones, the Python front ends exist - and the pieces of tests/test_coo_gpu.py that need no GPU hold: the row form as numpy states it,
and the array extraction, which hands over the triples of a scipy coo_matrix or a torch.sparse_coo_tensor as they stand."""
import os
import re
import subprocess

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd import _abi, engine_c
from test_abi_cpu import C_API_F90, HIP_C_F90, as_fortran_sees, c_class, fortran_procedures, mismatches, read, strip_c_comments, table_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fortran_davidson_amd", "lib")
EXT_H = os.path.join(ROOT, "include", "davidson_hip_ext.h")
CLASSES = ("banded", "random", "empty_rows", "missing_diagonal", "duplicates", "arrowhead")
ENTRIES = {"davx_set_operator_coo", "davx_set_operator_coo_dev"}
DOORS = {"fdx_engine_set_coo", "fdx_engine_set_coo_device"}


def exported(lib, prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return set(re.findall(rf"\s[TW]\s+({prefix}\w+)$", out, re.M))


def ext_prototypes():
    """name -> signature of every `int davx_name(args);` of the extension header"""
    return {name: ("i32", tuple(c_class(a.strip()) for a in args.split(",")))
            for name, args in re.findall(r"\bint\s+(davx_\w+)\s*\(([^()]*)\)\s*;", strip_c_comments(read(EXT_H)))}


def test_both_libraries_export_the_entries_and_the_doors():
    for lib in (os.path.join(LIBDIR, "libdavidson_hip.so"), os.path.join(LIBDIR, "test", "libdavidson_hip.so")):
        assert exported(lib, "davx_") == ENTRIES, lib
    assert exported(os.path.join(LIBDIR, "libfortran_davidson_amd.so"), "fdx_") == DOORS
    assert re.search(r"#define\s+DAV_HIP_ABI_VERSION\s+109\b", read(os.path.join(ROOT, "include", "davidson_hip.h")))
    assert "davx_" not in read(os.path.join(ROOT, "include", "davidson_hip.h"))          # ABI 109 itself: untouched
    # the device kernels are in the library
    syms = subprocess.run(["strings", os.path.join(LIBDIR, "libdavidson_hip.so")], capture_output=True, text=True, check=True).stdout
    for kernel in ("coo_check_kernel", "coo_scatter_kernel", "coo_sort_small_kernel", "coo_mark_kernel"):
        assert kernel in syms, kernel


def test_the_four_mirrors_of_the_extension_entries_are_equal():
    header = ext_prototypes()
    assert set(header) == ENTRIES
    assert header["davx_set_operator_coo"] == ("i32", ("ptr", "i32", "i64", "ptr", "ptr", "ptr", "i32", "i32"))
    assert header["davx_set_operator_coo_dev"] == ("i32", ("ptr", "i32", "i64", "ptr", "i32", "ptr", "i32", "ptr", "i32", "i32"))
    assert mismatches(header, table_signatures(_abi.EXT)) == []
    assert mismatches(header, fortran_procedures(read(HIP_C_F90), "davx_"), see=as_fortran_sees) == []
    doors = fortran_procedures(read(C_API_F90), "fdx_")
    assert set(doors) == DOORS and mismatches(doors, table_signatures(_abi.EXT_FD)) == []
    assert not set(_abi.EXT) & set(_abi.DAV) and not set(_abi.EXT_FD) & set(_abi.FD)
    # every davx_ / fdx_ call of the Python layer has its prototype
    pkg = os.path.join(ROOT, "fortran_davidson_amd")
    called = {name for f in os.listdir(pkg) if f.endswith(".py") for name in re.findall(r"\.((?:davx|fdx)_\w+)\(", read(os.path.join(pkg, f)))}
    assert called == ENTRIES | DOORS


def test_the_front_ends_exist():
    assert callable(fd.generalized_eigensolver_coo) and callable(fd.DavidsonEngine.set_coo)
    assert callable(fd.CEngine.set_operator_coo) and callable(fd.CEngine.set_operator_coo_dev)


def row_form(n, rows, cols, vals):
    """the definition, stated without a sort: entry k of row i is the k-th triple, in ascending p, whose row is i"""
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, np.asarray(rows) + 1, 1)
    indptr = np.cumsum(indptr)
    nxt = indptr[:-1].copy()
    ci, vv = np.zeros(len(rows), dtype=np.int32), np.zeros(len(rows))
    for p in range(len(rows)):
        q = nxt[rows[p]]
        nxt[rows[p]] += 1
        ci[q], vv[q] = cols[p], vals[p]
    return indptr, ci, vv


@pytest.mark.parametrize("kind", CLASSES)
def test_the_row_form_is_the_stable_sort_by_row(kind):
    from test_sparse_gpu import coo_to_csr, symmetric_coo
    n = 203
    rows, cols, vals = symmetric_coo(n, kind, np.random.default_rng(CLASSES.index(kind)))
    p = np.random.default_rng(1).permutation(len(rows))
    for r, c, v in ((rows, cols, vals), (rows[p], cols[p], vals[p]), (rows[::-1], cols[::-1], vals[::-1])):
        want, got = coo_to_csr(n, np.asarray(r), np.asarray(c), np.asarray(v, dtype=np.float64)), row_form(n, r, c, v)
        for a, b in zip(want, got):
            assert a.dtype == b.dtype and np.array_equal(a, b)


class Recorder:
    """an object with the attributes of a scipy coo_matrix whose conversions must not be called"""
    def __init__(self, row, col, data):
        self.row, self.col, self.data, self.shape = row, col, data, (4, 4)

    def tocsr(self):
        raise AssertionError("tocsr() must not be called on COO input")

    def sum_duplicates(self):
        raise AssertionError("sum_duplicates() must not be called on COO input")


def test_the_array_extraction_hands_over_duplicates_unsummed():
    row, col, data = np.array([2, 0, 2, 2, 1]), np.array([2, 0, 2, 1, 1]), np.array([1.0, 5.0, 2.0 ** -60, 0.5, -1.0])
    for m in [Recorder(row, col, data)]:
        ri, ci, vv = engine_c.coo_arrays(m)
        assert ri.dtype == np.int32 and ci.dtype == np.int32 and vv.dtype == np.float64
        assert np.array_equal(ri, row) and np.array_equal(ci, col) and np.array_equal(vv, data)
    sp = pytest.importorskip("scipy.sparse")
    m = sp.coo_matrix((data, (row, col)), shape=(4, 4))
    ri, ci, vv = engine_c.coo_arrays(m)
    assert vv.size == 5 and np.array_equal(ri, row) and np.array_equal(ci, col) and np.array_equal(vv, data)
    assert m.tocsr().nnz == 4          # ... which the library's own conversion would have summed


def test_a_torch_coo_tensor_is_read_uncoalesced():
    import torch
    idx = torch.tensor([[2, 0, 2, 2], [2, 0, 2, 1]])
    t = torch.sparse_coo_tensor(idx, torch.tensor([1.0, 5.0, 0.25, 0.5], dtype=torch.float64), size=(4, 4))
    assert not t.is_coalesced() and engine_c.is_torch_coo(t) and not engine_c.is_torch_csr(t)
    ri, ci, vv = engine_c.coo_arrays(t)
    assert ri.tolist() == [2, 0, 2, 2] and ci.tolist() == [2, 0, 2, 1] and vv.tolist() == [1.0, 5.0, 0.25, 0.5]
    parts = engine_c.coo_triples(idx[0], idx[1], torch.ones(4, dtype=torch.float64))          # three CPU tensors: the host path's arrays
    assert all(isinstance(a, np.ndarray) for a in parts) and parts[0].tolist() == [2, 0, 2, 2]
    with pytest.raises(ValueError, match="square"):
        engine_c.coo_arrays(torch.sparse_coo_tensor(idx, torch.ones(4, dtype=torch.float64), size=(4, 5)))


def test_the_python_checks_of_the_fortran_door():
    rows, cols, vals = np.array([0, 1, 2, 1]), np.array([0, 1, 2, 0]), np.ones(4)
    engine_c.check_coo(rows, cols, vals, 3, 0, True)
    with pytest.raises(ValueError, match=r"triple 3 at \(1, 3\) is out of range"):
        engine_c.check_coo(rows, np.array([0, 1, 2, 3]), vals, 3)
    with pytest.raises(ValueError, match=r"triple 1 at \(0, 1\) lies above the diagonal"):
        engine_c.check_coo(np.array([0, 0, 2]), np.array([0, 1, 2]), np.ones(3), 3, 0, True)
    with pytest.raises(ValueError, match="one length"):
        engine_c.check_coo(rows, cols[:3], vals, 3)
    with pytest.raises(ValueError, match="integers"):
        engine_c.check_coo(rows.astype(np.float64), cols, vals, 3)
    assert engine_c.coo_arrays(np.array([2 ** 40, -5, -2 ** 40]), np.array([0, 1, 2]), np.ones(3))[0].tolist() == [2 ** 31 - 1, -5, -2 ** 31]
