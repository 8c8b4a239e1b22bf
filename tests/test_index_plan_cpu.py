"""CPU: the incremental index's host plan (needle_amd/csrc/index_plan.h), compiled for the host with nothing of ROCm on the
include path.  tests/cpp/index_plan_check.cpp holds the plan of lists without labels against the expressions index.cpp had
before (every n0 + k <= 40, one and two regions), labelled lists against brute force, one label against none, the ids and
their inverse (also where pairs x regions crosses 0xFFFFFFF0), appends in one step against appends in several, edits
against index.cpp's former loops and brute force, the min_len bound of both streamed routes, and the acceptance chains of
add_matched, add_matched_grouped and add_streamed fact by fact, with the refusals' words.  Once as it is and once under
AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_index_plans(tmp_path, flags):
    exe = str(tmp_path / "index_plan_check")
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "needle_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "index_plan_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("index plan ok"), out.stdout[-4000:] + out.stderr[-4000:]
