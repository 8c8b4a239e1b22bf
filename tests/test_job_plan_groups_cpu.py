"""CPU: the plan of a library job over groups of videos (needle_amd/csrc/job_plan.h, JobShape::pairs), compiled for the host
with nothing of ROCm on the include path.  tests/cpp/job_plan_groups_check.cpp plans jobs for worlds 1, 2, 3, 5 and 8 and
grouped pair counts 0, 1, 6, 16 383, 16 384 and 65 536 and asserts that the ranks' pair ranges cover [0, P) exactly once,
that every rank derives the same form and the same verdicts from the same history, that the form follows the pair count,
and that a shape whose pair count is job_pairs(n) plans what the plain shape plans, field for field.  Once as it is and
once under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_grouped_job_plans(tmp_path, flags):
    exe = str(tmp_path / "job_plan_groups_check")
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "needle_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "job_plan_groups_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("job plan groups ok"), out.stdout[-4000:] + out.stderr[-4000:]
