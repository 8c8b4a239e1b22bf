"""The library of tests/test_gpu_library_groups.py and tests/test_gpu_library_groups_ranks.py -- eight episodes in two seasons
of three with scattered members and two videos alone -- and one rank of the multi-process run over it:

  library_groups_worker.py <out> : needle_hip_comm_init, Library.set_groups + set_pcm (the PCM of this rank's own block),
                                   three pipelined job_begin / job_end; writes every job's results, run count, form, what
                                   its collectives moved and the runs this rank holds afterwards.

Seasons 5 and 9 are cut from ONE seed base with disjoint episode indices: every episode carries the same intro, so a
search over the whole list matches across the seasons; only the labels keep them apart."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from needle_amd import capi, rendezvous, synth  # noqa: E402

LABELS = [5, 9, 5, 7, 9, 5, 3, 9]                        # seasons {0, 2, 5} and {1, 4, 7}; videos 3 and 6 alone: 6 pairs
SECONDS = [66.0 + 3.0 * k for k in range(8)]             # ragged: 66 .. 87 s
INTRO_S = 20.0


def episode(k):
    return synth.make_episode(k, SECONDS[k], INTRO_S)


def totals():
    return [int(round(s * synth.RATE)) for s in SECONDS]


def members_of(labels):
    """label -> list positions in ascending order, labels in the order of their first appearance"""
    groups = {}
    for v, g in enumerate(labels):
        groups.setdefault(g, []).append(v)
    return groups


def comparator(n=8):
    return capi.Comparator([f"ep{k}.wav" for k in range(n)], min_opening_duration=10)


def _res(rs):
    return [None if r is None else [None if r.opening is None else list(r.opening),
                                    None if r.ending is None else list(r.ending)] for r in rs]


def main(out):
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    rdzv = rendezvous.init_comm(capi, rank, world, int(os.environ.get("LOCAL_RANK", "0")),
                                key=os.environ["NEEDLE_TEST_RDZV_KEY"])
    n = len(LABELS)
    lib = capi.Library(n).set_groups(LABELS)
    first, count = lib.rank_videos(totals(), world, rank)        # does not depend on the labels
    mine = {k: episode(k) for k in range(first, first + count)}
    lib.set_pcm([mine[k].pcm if k in mine else None for k in range(n)], totals())
    cmp = comparator(n)
    jobs = []

    def end(slot):
        res, found = lib.job_end(cmp, slot)
        held = lib.job_runs(slot)
        jobs.append({"results": _res(res), "runs": found, "form": lib.job_form(slot), "comm": lib.job_comm_bytes(slot),
                     "held": sorted([int(r["problem"]), int(r["src_end"]), int(r["dst_end"]), int(r["len"])] for r in held)})

    lib.job_begin(cmp, 0)
    lib.job_begin(cmp, 1)
    end(0)
    lib.job_begin(cmp, 0)
    end(1)
    end(0)
    with open(f"{out}.{rank}", "w") as f:
        json.dump({"rank": rank, "backend": capi.comm_backend(), "world": capi.comm_world_size(), "pairs": lib.num_pairs(),
                   "groups": lib.groups(), "pair_range": list(capi.comm_shard(lib.num_pairs(), world, rank)),
                   "video_block": list(capi.comm_shard(n, world, rank)), "jobs": jobs}, f)
    capi.comm_barrier()
    capi.comm_finalize()
    rdzv.close()


if __name__ == "__main__":
    main(sys.argv[1])
