"""CPU: the table of correction methods - names, codes, what each method needs - says the same in every layer, checked through the code of
each layer and not through its text: the Python parser and checks, the Fortran module davidson_method (tests/fortran/prog_methods.f90)
and the C header (tests/helpers/method_codes.c).  tests/method_table.json holds what the commit before the table existed answered -
solver._method_code, every refusal of the front ends and of the three _check_* functions word for word, the Fortran driver's parser and
the doors' method_label - so the comparison is with recorded behaviour, not with a restatement of the code under test."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import fortran_davidson_amd as fd
from fortran_davidson_amd import engine_c, solver
import bdpr_inputs as BI
import cheb_inputs as CI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC = "/opt/rocm/lib/llvm/bin/flang"

NAMES = ["DPR", "GJD", "BDPR", "CHEB", "CHEB1", "CHEB16", "CHEB64", "CHEB0", "CHEB65", "CHEBx", "CHEB-1", "CHEB1.5", "CHEB 4", "LCHEB",
         "LCHEB1", "LCHEB16", "LCHEB64", "LCHEB0", "LCHEB65", "LCHEBx", "LCHEB123", "LCHE", "nonsense", "", "dpr", "Cheb"]
CODES = [0, 1, 2, 3, 4, 5, 6, 255, 256, 260, 1282, 4100, 4101, 16644]

with open(os.path.join(ROOT, "tests", "method_table.json")) as _f:
    TABLE = json.load(_f)


class _NoCalls:
    """a library stand-in whose every symbol fails the test when called"""
    def __getattr__(self, name):
        def call(*args):
            raise AssertionError(f"{name} was called")
        return call


def outcome(thunk):
    """what a call answers, as the table records it: its value, or the class and the full text of what it raises"""
    try:
        return {"returns": thunk()}
    except Exception as exc:        # noqa: BLE001 - the class is part of the record
        return {"raises": type(exc).__name__, "text": str(exc)}


def refusal_cases(solver, fd):
    """the cases of the three test_front_ends_refuse_before_any_engine_call tests (test_bdpr_cpu, test_cheb_cpu, test_lcheb_cpu), by
    name: the front ends, the three _check_* functions and DavidsonEngine.solve.  `solver.fortran_lib` is a _NoCalls while they run."""
    cases = {}
    ab, bm = BI.block_matrix(24, 4, 1, gev=True)
    brp, bci, bvv = BI.bsr_of(ab, 4)
    brp2, bci2, bvv2 = BI.bsr_of(bm, 2)
    a = CI.laplacian2d(5, 1)
    rp, ci, vv = CI.csr_of(a)
    v3 = vv.reshape(-1, 1, 1)
    S = solver
    cases["dense BDPR"] = lambda: S.generalized_eigensolver(ab, 2, "BDPR", 10, 1e-8)
    cases["sparse BDPR"] = lambda: S.generalized_eigensolver_sparse(np.arange(25), np.arange(24), np.ones(24), 2, "BDPR", 10, 1e-8)
    cases["bsr BDPR B of another block size"] = lambda: S.generalized_eigensolver_bsr(brp, bci, bvv, 2, "BDPR", 10, 1e-8,
                                                                                        second=(brp2, bci2, bvv2))
    cases["bsr BDPR flat blocks"] = lambda: S.generalized_eigensolver_bsr(brp, bci, bvv.reshape(-1, 16), 2, "BDPR", 10, 1e-8)
    cases["bsr BDPR n=26"] = lambda: S.generalized_eigensolver_bsr(brp, bci, bvv, 2, "BDPR", 10, 1e-8, n=26)
    cases["bsr BDPR float32 guess"] = lambda: S.generalized_eigensolver_bsr(brp, bci, bvv, 2, "BDPR", 10, 1e-8,
                                                                             initial_vectors=np.ones((24, 2), dtype=np.float32))
    cases["bsr BDPR short guess"] = lambda: S.generalized_eigensolver_bsr(brp, bci, bvv, 2, "BDPR", 10, 1e-8, initial_vectors=np.ones((23, 2)))
    for method in ("CHEB", "CHEB16", "LCHEB", "LCHEB16"):
        cases[f"dense {method}"] = lambda m=method: S.generalized_eigensolver(a, 2, m, 10, 1e-8)
        cases[f"dense {method} gev"] = lambda m=method: S.generalized_eigensolver(a, 2, m, 10, 1e-8, None, np.eye(25))
        cases[f"free {method}"] = lambda m=method: S.generalized_eigensolver_free(lambda x: a @ x, 25, 2, m, 10, 1e-8, 20, lambda x: x)
        cases[f"sparse {method} gev"] = lambda m=method: S.generalized_eigensolver_sparse(rp, ci, vv, 2, m, 10, 1e-8, second=(rp, ci, vv))
        cases[f"bsr {method} gev"] = lambda m=method: S.generalized_eigensolver_bsr(rp, ci, v3, 2, m, 10, 1e-8, second=(rp, ci, v3))
    for method in ("CHEB65", "CHEB0", "LCHEB65", "LCHEB0", "CHEBx", "LCHEB1.5"):
        cases[f"dense {method}"] = lambda m=method: S.generalized_eigensolver(a, 2, m, 10, 1e-8)
        cases[f"free {method}"] = lambda m=method: S.generalized_eigensolver_free(lambda x: a @ x, 25, 2, m, 10, 1e-8, 20, lambda x: x)
        cases[f"sparse {method}"] = lambda m=method: S.generalized_eigensolver_sparse(rp, ci, vv, 2, m, 10, 1e-8)
        cases[f"bsr {method}"] = lambda m=method: S.generalized_eigensolver_bsr(rp, ci, v3, 2, m, 10, 1e-8)
    # the three checks, called as the tests before called them
    for name, args, kw in (("DPR", ((None, None),), {}), ("GJD", ((None, 4),), {"gev": True}), ("BDPR", ((4, None),), {}),
                           ("BDPR", ((4, 4),), {"gev": True}), ("BDPR", ((5, None),), {"n": 240, "nranks": 3}), ("BDPR", ((None, None),), {}),
                           ("BDPR", ((4, None),), {"gev": True}), ("BDPR", ((4, 2),), {"gev": True}),
                           ("BDPR", ((3, None),), {"n": 240, "nranks": 3}), ("BDPR", ((3, None), False, 240, 3, "DavidsonEngine.solve"), {}),
                           ("CHEB99", ((None, None),), {}), ("LCHEB99", ((None, None),), {})):
        cases[f"_check_bdpr {name} {args} {kw}"] = lambda n=name, a_=args, k=kw: S._check_bdpr(n, *a_, **k)
    for name, args, kw in (("DPR", (False,), {}), ("GJD", (False,), {"gev": True}), ("BDPR", (False,), {}), ("CHEB", (True,), {}),
                           ("CHEB33", (True,), {}), ("CHEB", (False,), {}), ("CHEB12", (True,), {"gev": True}),
                           ("CHEB12", (False, True, "somewhere"), {}), ("CHEB99", (True,), {}), ("LCHEB99", (False,), {}),
                           ("LCHEB", (False,), {"gev": True})):
        cases[f"_check_cheb {name} {args} {kw}"] = lambda n=name, a_=args, k=kw: S._check_cheb(n, *a_, **k)
    for name, args, kw in (("DPR", (), {"gev": True, "host_callbacks": True}), ("GJD", (), {"gev": True, "host_callbacks": True}),
                           ("BDPR", (), {"gev": True, "host_callbacks": True}), ("CHEB", (), {"gev": True, "host_callbacks": True}),
                           ("CHEB12", (), {"gev": True, "host_callbacks": True}), ("LCHEB", (), {}), ("LCHEB33", (), {}),
                           ("LCHEB12", (), {"gev": True}), ("LCHEB12", (True, True, "somewhere"), {}), ("LCHEB", (False, True), {}),
                           ("LCHEB99", (), {}), ("CHEB99", (), {"gev": True})):
        cases[f"_check_lcheb {name} {args} {kw}"] = lambda n=name, a_=args, k=kw: S._check_lcheb(n, *a_, **k)

    # the resident engine: what its operators are is known from the set calls
    class Eng(fd.DavidsonEngine):
        def __init__(self, gev=False, nranks=1, notes=()):
            self.lib, self.gev, self.n, self.nranks, self.lowest, self.max_dim, self.p = _NoCalls(), gev, 240, nranks, 2, 20, None
            for note in notes:
                self._note_blocks(*note[0], **note[1])

    def solve(method, **kw):
        return lambda: Eng(**kw).solve(method)[2]
    sparse_then_not = (((1, None), {"sparse": True}), ((1, None), {}))
    cases["engine CHEB nothing set"] = solve("CHEB")
    cases["engine CHEB8 no longer sparse"] = solve("CHEB8", notes=sparse_then_not)
    cases["engine CHEB bsr gev"] = solve("CHEB", gev=True, notes=(((1, 4), {}),))
    cases["engine CHEB bsr"] = solve("CHEB", notes=(((1, 4), {}),))
    cases["engine CHEB70 csr"] = solve("CHEB70", notes=(((1, None), {"sparse": True}),))
    cases["engine LCHEB gev"] = solve("LCHEB", gev=True)
    cases["engine LCHEB99"] = solve("LCHEB99")
    cases["engine LCHEB16"] = solve("LCHEB16")
    cases["engine BDPR nothing set"] = solve("BDPR")
    cases["engine BDPR B not bsr"] = solve("BDPR", gev=True, notes=(((1, 4), {}),))
    cases["engine BDPR B of block size 2"] = solve("BDPR", gev=True, notes=(((1, 4), {}), ((2, 2), {})))
    cases["engine BDPR 3 ranks b=3"] = solve("BDPR", nranks=3, notes=(((1, 3), {}),))
    cases["engine BDPR 3 ranks b=5"] = solve("BDPR", nranks=3, notes=(((1, 5), {}),))
    cases["engine DPR"] = solve("DPR")
    cases["engine nonsense"] = solve("nonsense")
    return cases


# ---- 1. Python -----------------------------------------------------------------------------------------------------------------------
def test_python_method_codes_are_the_recorded_ones():
    assert sorted(TABLE["python_codes"]) == sorted(NAMES)
    for name in NAMES:
        assert outcome(lambda: solver._method_code(name)) == TABLE["python_codes"][name], name
    assert solver._METHOD == {"DPR": 0, "GJD": 1, "BDPR": 3}
    for name in NAMES:
        want = TABLE["python_codes"][name]
        if "returns" in want:
            kind, degree = solver._parse_method(name)
            assert kind | degree << 8 == want["returns"] and engine_c.method_code(kind, degree) == want["returns"], name
    assert engine_c.method_cheb() == 4 and engine_c.method_cheb(16) == 4100 and engine_c.method_lcheb() == 5 and engine_c.method_lcheb(16) == 4101
    assert (engine_c.METHOD_DPR, engine_c.METHOD_GJD, engine_c.METHOD_NONE, engine_c.METHOD_BDPR, engine_c.METHOD_CHEB,
            engine_c.METHOD_LCHEB) == (0, 1, 2, 3, 4, 5)


def test_every_refusal_is_the_recorded_one_word_for_word(monkeypatch):
    monkeypatch.setattr(solver, "fortran_lib", lambda: _NoCalls())
    cases = refusal_cases(solver, fd)
    assert sorted(cases) == sorted(TABLE["refusals"])
    for name, thunk in cases.items():
        assert outcome(thunk) == TABLE["refusals"][name], name
    # every kind of answer is among them: nothing to refuse, a refusal, and the first engine call reached
    kinds = {(v.get("raises"), "returns" in v) for v in TABLE["refusals"].values()}
    assert {("ValueError", False), ("TypeError", False), ("AssertionError", False), (None, True)} <= kinds


# ---- 2. Fortran and C ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fortran_answers(tmp_path_factory):
    """tests/fortran/prog_methods.f90 run once: ({name: (code, label, kind, block_in_ritz_phase)}, {code: (label, kind)}, message)"""
    if not os.path.exists(FC):
        pytest.skip("flang not available")
    from test_fortran_programs import SRC, compile_link
    tmp = tmp_path_factory.mktemp("prog_methods")
    exe = compile_link([os.path.join(SRC, "prog_methods.f90")], str(tmp / "prog_methods"), tmp)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    names = {n: (int(c), lab, int(k), b == "T") for n, c, lab, k, b in re.findall(r"^NAME \[(.*?)\] (-?\d+) \[(.*?)\] (-?\d+) ([TF])$", out, re.M)}
    codes = {int(c): (lab, int(k)) for c, lab, k in re.findall(r"^CODE (-?\d+) \[(.*?)\] (-?\d+)$", out, re.M)}
    return names, codes, out[out.index("MESSAGE\n") + len("MESSAGE\n"):]


def test_the_fortran_module_answers_as_the_driver_and_the_doors_did(fortran_answers):
    names, codes, message = fortran_answers
    rec = TABLE["fortran"]
    assert sorted(names) == sorted(NAMES) == sorted(rec["names"]) and sorted(codes) == CODES == sorted(int(c) for c in rec["codes"])
    for name in NAMES:
        code, label, kind, block = names[name]
        want = rec["names"][name]
        assert code == want["code"], name
        if code >= 0:
            # the inverse, the engine's kind, and the side of the loop the method takes
            assert (label, kind, block) == (want["label"], want["kind"], want["block_in_ritz_phase"]), name
            assert label == name
    for code in CODES:
        assert codes[code] == (rec["codes"][str(code)]["label"], rec["codes"][str(code)]["kind"]), code
    # names no method has: the doors hand the driver a name it refuses
    for code in (2, 6, 255, 256, 1282, 16644):
        assert names.get(codes[code][0], (-1,))[0] == -1, code
    assert message == rec["unknown_message"]


def test_the_fortran_parser_agrees_with_the_python_one(fortran_answers):
    """(moved here from test_lcheb_cpu.py with its expectations; the program now prints one code per name, so a pair (lcheb code, cheb
    code) of that test is the code where the name is of that family and -1 otherwise)"""
    names = fortran_answers[0]
    want = {"LCHEB": (5, -1), "LCHEB16": (5 + 16 * 256, -1), "LCHEB1": (261, -1), "LCHEB64": (5 + 64 * 256, -1), "LCHEB0": (-1, -1),
            "LCHEB65": (-1, -1), "LCHEBx": (-1, -1), "LCHEB123": (-1, -1), "CHEB": (-1, 4), "CHEB16": (-1, 4100), "LCHE": (-1, -1),
            "DPR": (-1, -1)}
    for name, (lcode, ccode) in want.items():
        code = names[name][0]
        got = (code if name.startswith("L") and code >= 0 else -1, code if name.startswith("C") and code >= 0 else -1)
        assert got == (lcode, ccode), name
        if lcode >= 0:
            assert solver._method_code(name) == lcode
    assert names["DPR"][0] == 0
    # where both accept a name the codes are equal, and Python accepts exactly the names Fortran accepts (what Python does not raise on
    # and does not know is code 2, the name the driver refuses)
    for name in NAMES:
        py = outcome(lambda: solver._method_code(name))
        accepted = "returns" in py and py["returns"] != 2
        assert accepted == (names[name][0] >= 0), name
        if accepted:
            assert py["returns"] == names[name][0], name


def test_the_header_has_the_same_codes(tmp_path, fortran_answers):
    exe = str(tmp_path / "method_codes")
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "helpers", "method_codes.c"), "-o", exe],
                   check=True, capture_output=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [0, 1, 2, 3, 4, 5, 4100, 4101]
    assert got[:6] == [engine_c.METHOD_DPR, engine_c.METHOD_GJD, engine_c.METHOD_NONE, engine_c.METHOD_BDPR, engine_c.METHOD_CHEB,
                       engine_c.METHOD_LCHEB]
    assert got[6:] == [engine_c.method_cheb(16), engine_c.method_lcheb(16)] == [solver._method_code("CHEB16"), solver._method_code("LCHEB16")]
    names = fortran_answers[0]
    assert [names[n][0] for n in ("DPR", "GJD", "BDPR", "CHEB", "LCHEB", "CHEB16", "LCHEB16")] == got[:2] + got[3:]
