"""Records tests/golden/outer_loop_footprints.json: the footprint of every case of tests/outer_loop_cases.py, on the GPU.

Run it with the package of the PARENT of the commit under test first on the path - that commit built side by side in a scratch
worktree:

    PYTHONPATH=<parent worktree> python tests/record_outer_loop.py [--compare]

It refuses to write the fixture when a case misses the condition its entry states (a case could then silently miss its branch).
--compare: writes nothing, runs the cases with the package it finds and reports, per case, whether integers and eigenvalues equal the
fixture's bit for bit - the check of the recording session, made with the commit under test on the path."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)                              # the case list: this tree's
sys.path.append(os.path.dirname(HERE))                # the package: PYTHONPATH's first, this tree's when there is none
FIXTURE = os.path.join(HERE, "golden", "outer_loop_footprints.json")

# the test build of the engine that belongs to the package about to be imported (tests/conftest.py does the same for pytest)
_pkg = os.path.dirname(importlib.util.find_spec("fortran_davidson_amd").origin)
_test_lib = os.path.join(_pkg, "lib", "test", "libdavidson_hip.so")
if os.path.exists(_test_lib):
    os.environ.setdefault("DAVIDSON_HIP_LIB", _test_lib)

import fortran_davidson_amd as fd                     # noqa: E402
import outer_loop_cases as OL                         # noqa: E402


def footprints():
    out = {}
    for name, c in OL.CASES.items():
        saved = {k: os.environ.get(k) for k in c["env"]}
        os.environ.update(c["env"])
        try:
            out[name] = OL.run_case(c, fd)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        print(name, out[name], flush=True)
    return out


def main():
    print("package:", _pkg)
    found = footprints()
    if "--compare" in sys.argv:
        with open(FIXTURE) as f:
            want = json.load(f)
        differ = [name for name in OL.CASES if found[name] != want[name]]
        print("bit for bit equal to the fixture:", len(OL.CASES) - len(differ), "of", len(OL.CASES), "cases; different:", differ)
        return 1 if differ else 0
    missed = [name for name, c in OL.CASES.items() if c["check"] is not None and not c["check"](found[name])]
    if missed:
        print("NOT written - cases that miss their condition:", missed)
        return 1
    with open(FIXTURE, "w") as f:
        json.dump(found, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)
    return 0


if __name__ == "__main__":
    sys.exit(main())
