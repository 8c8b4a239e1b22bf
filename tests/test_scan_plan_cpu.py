"""CPU: the all-pairs scan's launch plan (needle_amd/csrc/scan_plan.h), compiled for the host -- tests/cpp/scan_plan_check.cpp
builds plans for synthetic tables that take every branch of the planner (kernel choice at min_len 20 .. 23, the automatic
matrix pipe at 2047 / 2048 pairs and on badly filled row tiles, its forced form at every workgroup shape, split count and LDS
budget, the oversize partition, window images up to and beyond 2 GB, the growth of bands per wave, the refusals), asserts what
the kernels rely on for each, and prints one line per plan.  The lines are compared with tests/golden/scan_plans.txt, recorded
from the planner as one function, before it was taken apart into stages: a plan that changes for any of these inputs, a packing
that breaks, shows here and not as a fault on a GPU.  Once as it is and once under AddressSanitizer and
UndefinedBehaviorSanitizer (a stand-alone program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_scan_plans_against_the_recorded_ones(tmp_path, flags):
    exe = str(tmp_path / "scan_plan_check")
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "needle_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "scan_plan_check.cpp")], check=True)
    out = subprocess.run([exe, "--record"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("scan plans ok"), out.stdout[-4000:] + out.stderr[-4000:]
    with open(os.path.join(ROOT, "tests", "golden", "scan_plans.txt")) as f:
        want = f.read().splitlines()
    got = out.stdout.splitlines()[:-1]
    assert len(got) == len(want) and len(want) > 40
    for g, w in zip(got, want):
        assert g == w
