"""CPU: the grouped pair numbering of needle_amd/csrc/pair_ids.h (groups of videos: only pairs inside a group have an id),
compiled for the host -- tests/cpp/group_ids_check.cpp against the enumeration itself, once as it is and once under
AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: the tables are indexed by what the labels say)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_group_ids_against_the_enumeration(tmp_path, flags):
    """Every partition of up to 7 videos, 300 random label vectors of up to 600, one group of 258: id <-> (a, b), density, one
    group == i-major, every video's slots its group partners in the reference's order."""
    exe = str(tmp_path / "group_ids_check")
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "needle_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "group_ids_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("group ids ok"), out.stdout + out.stderr
