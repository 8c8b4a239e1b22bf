"""CPU: what the ranks of a library job send each other (needle_amd/csrc/job_plan.h), compiled for the host with nothing of
ROCm on the include path -- tests/cpp/job_plan_check.cpp plans jobs for synthetic shapes, switches and histories (form: the
device epilogue's thresholds by pairs and by the last job's count, one and two videos, every switch, the sharding threshold,
worlds 1 .. 65, arena against comparator regions, the epilogue failing on one rank; sizes: a first job, the 1 MiB rule, the
forced head and slab, round_up4's clamp, the head from the last count; directed: no matrix yet, a matrix of another world,
ragged matrices, the forced cap once and not twice, no point-to-point transport, blocks beyond 4 GiB; verdict: the largest
count around the head and the slab, a block at and beyond its cap, a slab overflow, a form that changes at the repeat; end:
job_end's decision to gather result blocks around 131 072 runs, with the switch, with a form fixed at the enqueue),
asserts for every rank of every case what the executor and the transport rely on (the same plan and verdict everywhere, send
and receive sizes that meet, blocks that tile, multiples of 4, a repeat loop that ends, what each verdict leaves of the count
matrix), and prints one line per case: the first attempt's plan, every attempt's form, the verdicts, the history left.

The program also carries the expressions as they stood in library.cpp before job_plan.h existed (its namespace `before`)
and runs them beside the new ones for every rank and every attempt: plan, verdict and history must agree.  The lines are
compared with tests/golden/job_plans.txt, recorded from this program; that the old expressions give the same plans is what
the program asserts, not something the file's history shows.  Once as it is and once under AddressSanitizer and
UndefinedBehaviorSanitizer (a stand-alone program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAMILIES = """form/pairs form/pairs-regions form/last-count form/n form/switches form/shard-threshold form/shard-threshold-pairs
form/world form/world-history form/regions form/epilogue-fails-on-one-rank
sizes/first-job sizes/one-mib sizes/forced-head sizes/forced-slab sizes/round-up4-clamp sizes/head-from-last-count
directed/no-matrix directed/matrix-of-another-world directed/ragged directed/ragged-large directed/unsupported
directed/forced-cap directed/beyond-4-gib
verdict/largest-count verdict/largest-count-counted verdict/largest-count-directed verdict/block
verdict/slab-overflow-clears-the-matrix verdict/form-changes-at-the-repeat end/sharded""".split()


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_job_plans_against_the_recorded_ones(tmp_path, flags):
    exe = str(tmp_path / "job_plan_check")
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "needle_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "job_plan_check.cpp")],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("job plans ok"), out.stdout[-4000:] + out.stderr[-4000:]
    with open(os.path.join(ROOT, "tests", "golden", "job_plans.txt")) as f:
        want = f.read().splitlines()
    got = out.stdout.splitlines()[:-1]
    assert {line.split(":")[0] for line in got} >= set(FAMILIES)
    assert len(got) == len(want) and len(want) > 150
    for g, w in zip(got, want):
        assert g == w
