"""The outer loop's footprints (tests/outer_loop_cases.py) against the fixture recorded from the loop as it stood before it was split
into named steps (tests/record_outer_loop.py; tests/golden/outer_loop_footprints.json): per case the iteration count and - on a resident
engine - the engine's counters after reset_stats() (operator applies, their columns and launches, restarts, collectives, the final basis
width), every integer equal; the eigenvalues to the absolute bound tests/test_solver_gpu.py applies to its goldens (not bit for bit:
host LAPACK may take another code path on another host CPU)."""
import json
import os

import numpy as np
import pytest

import fortran_davidson_amd as fd
import outer_loop_cases as OL

pytestmark = pytest.mark.gpu
EV_TOL = 1e-8


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outer_loop_footprints.json")) as f:
        return json.load(f)


def test_fixture_holds_every_case_and_its_condition(recorded):
    assert sorted(recorded) == sorted(OL.CASES)
    for name, c in OL.CASES.items():
        assert set(recorded[name]) == {"iters", "eigenvalues"} | (set(OL.COUNTERS) if c["counters"] else set()), name
        assert c["check"] is None or c["check"](recorded[name]), name


@pytest.mark.parametrize("name", sorted(OL.CASES))
def test_outer_loop_leaves_the_recorded_footprint(recorded, name, monkeypatch):
    c = OL.CASES[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    found, want = OL.run_case(c, fd), recorded[name]
    print(name, found)
    for k in want:
        if k != "eigenvalues":
            assert found[k] == want[k], (name, k, found[k], want[k])
    assert np.abs(np.array(found["eigenvalues"]) - np.array(want["eigenvalues"])).max() < EV_TOL
