"""The kernel trace of one run of tests/test_exact_phases_gpu.py (profiles/exact_phases_kernel_coverage.csv, rocprofv3 --kernel-trace
--stats) shows a launch of every kernel instantiation in that module's dispatch table."""
import csv
import os

from test_exact_phases_gpu import DISPATCH

CSV = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "exact_phases_kernel_coverage.csv")


def test_every_kernel_in_the_dispatch_table_was_launched():
    with open(CSV, newline="") as f:
        calls = {row["Name"]: int(row["Calls"]) for row in csv.DictReader(f)}
    missing = [inst for inst in DISPATCH if not any(inst + "(" in name and n > 0 for name, n in calls.items())]
    assert not missing, missing
