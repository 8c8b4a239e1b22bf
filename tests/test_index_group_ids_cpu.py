"""CPU: the index store's grouped, append-stable pair numbering of needle_amd/csrc/pair_ids.h (IndexGroupView), compiled for
the host -- tests/cpp/index_group_ids_check.cpp against a brute-force enumeration, once as it is and once under
AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: the tables are indexed by what the labels say)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_index_group_ids_against_the_enumeration(tmp_path, flags):
    """400 random label lists of 0 to 40 videos and 1 to 8 labels, all in one group, every video alone: id <-> (a, b), every
    id hit once, one group == column-major, every video's slots in the reference's order over its group, and every pair of
    every prefix keeps its id in the whole list."""
    exe = str(tmp_path / "index_group_ids_check")
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "needle_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "index_group_ids_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("index group ids ok"), out.stdout + out.stderr
