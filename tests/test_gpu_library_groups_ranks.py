"""GPU tests (-m gpu) of a library job over groups of videos between ranks: real processes (tests/library_groups_worker.py)
that share device 0 over the host-staged transport, worlds 2, 3 and 5 -- at most 5 processes with the GPU open beside this
one.  The oracle is the checker: every rank's results of every job equal O.run_with_frame_hashes over each season's own
sub-list.

Eight videos, labels [5, 9, 5, 7, 9, 5, 3, 9], 6 grouped pairs.  With three ranks the video blocks {0, 1, 2}, {3, 4, 5},
{6, 7} cut through both seasons; with five the pair ranges are 2, 2, 2, 0, 0 (two ranks scan nothing) and the last rank's
block of videos is empty.  In the `directed` cases the third job's runs travel owner-directed: the kernel that sorts them
by destination decodes grouped pair ids from the device tables, and the epilogue runs sharded by video on the device.
The overflow case runs with two ranks: the six pairs have 10 runs, and only there does one block get more than the 4 runs
of a forced block (the test asserts that premise from the run list itself)."""
import json
import os
import socket
import subprocess
import sys
import time
import uuid

import pytest

from needle_amd import capi
from oracle import oracle as O
from tests import library_groups_worker as W

pytestmark = pytest.mark.gpu
NS = O.NS
HERE = os.path.dirname(os.path.abspath(__file__))
LABELS = W.LABELS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch(world, out, extra_env, timeout=300):
    """One worker per rank, every rank on device 0.  A rank that fails ends the launch at once (the others would wait for it
    in a collective); a launch that outlives `timeout` seconds is killed."""
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               NEEDLE_TEST_RDZV_KEY=uuid.uuid4().hex, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.update(extra_env)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "library_groups_worker.py"), out],
                              env=dict(env, RANK=str(rank), LOCAL_RANK="0")) for rank in range(world)]
    deadline = time.monotonic() + timeout
    try:
        while any(p.poll() is None for p in procs):
            if any(p.poll() not in (None, 0) for p in procs) or time.monotonic() > deadline:
                break
            try:
                next(p for p in procs if p.poll() is None).wait(timeout=0.2)
            except subprocess.TimeoutExpired:
                pass
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    codes = [p.returncode for p in procs]
    assert codes == [0] * world, codes
    return [json.load(open(f"{out}.{r}")) for r in range(world)]


@pytest.fixture(scope="module")
def want():
    """The per-season oracle, computed once."""
    hd = O.duration_from_secs_f32(0.3)
    eps = [W.episode(k) for k in range(8)]
    ref = O.analyze_batch([e.pcm[: len(e.pcm) // 2] for e in eps], 1, hd)
    ocmp = O.Comparator(min_opening_duration=10 * NS)
    out = [None] * 8
    for members in W.members_of(LABELS).values():
        if len(members) >= 2:
            for v, r in zip(members, O.run_with_frame_hashes(ocmp, [ref[v] for v in members])):
                out[v] = None if r is None else [None if r.opening is None else list(r.opening),
                                                 None if r.ending is None else list(r.ending)]
    assert out[3] is None and out[6] is None and all(out[v] is not None and out[v][0] is not None for v in (0, 1, 2, 4, 5, 7))
    return out


CASES = [(2, "0", None), (3, "1", None), (5, "1", None), (2, "directed", None), (3, "directed", None), (5, "directed", None),
         (2, "directed-overflow", None), (3, "directed", 4), (2, "1", 4)]


@pytest.mark.parametrize("world,shard_epilogue,slab_runs", CASES)
def test_grouped_ranks_over_host_transport_on_one_gpu(want, tmp_path, world, shard_epilogue, slab_runs):
    env = {"NEEDLE_HIP_COMM": "host", "NEEDLE_HIP_SHARD_EPILOGUE": shard_epilogue}
    directed = shard_epilogue.startswith("directed")
    if directed:                                   # the sharded DEVICE epilogue at this small size
        env.update(NEEDLE_HIP_SHARD_EPILOGUE="1", NEEDLE_HIP_DEVICE_EPILOGUE="1")
    if shard_epilogue == "directed-overflow":      # ... into blocks of 4 runs the first time: the sizes grow, once more
        env.update(NEEDLE_HIP_TEST_DIRECTED_CAP="4")
    if slab_runs:
        env["NEEDLE_HIP_SLAB_RUNS"] = str(slab_runs)
    got = launch(world, str(tmp_path / "r"), env)
    pairs = [tuple(p) for p in capi.group_pairs(LABELS).tolist()]
    assert len(pairs) == 6
    block = -(-8 // world)
    for rank, g in enumerate(got):
        assert g["rank"] == rank and g["backend"] == "host" and g["world"] == world
        assert g["pairs"] == 6 and g["groups"] == LABELS
        assert g["video_block"] == [min(rank * block, 8), max(0, min(block, 8 - rank * block))]
        for job in g["jobs"]:
            assert job["results"] == want, (rank, job["form"])
            assert job["runs"] == got[0]["jobs"][0]["runs"] >= 6
            assert all(run[0] < 6 for run in job["held"])
            assert job["form"]["sharded_epilogue"] is (shard_epilogue != "0")
            assert job["form"]["device_epilogue"] is directed
    assert sum(g["pair_range"][1] for g in got) == 6
    if world == 5:
        assert [g["pair_range"][1] for g in got] == [2, 2, 2, 0, 0] and got[4]["video_block"][1] == 0
    if world == 3:
        assert [g["video_block"] for g in got] == [[0, 3], [3, 3], [6, 2]]
    everything = got[0]["jobs"][0]["held"]
    assert len(everything) == got[0]["jobs"][0]["runs"]
    if not directed:
        for g in got:
            assert all(job["held"] == everything and not job["form"]["directed_runs"] for job in g["jobs"])
        return
    # jobs 0 and 1 were in flight before any count matrix existed (heads: a rank holds every run); job 2 went owner-directed:
    # a rank holds the runs of pairs with a video in its block, and nothing else -- all ranks together every run at least once
    if shard_epilogue == "directed-overflow":
        # the premise: some rank directs more than the 4 runs of a forced block to some rank (two ranks: rank 1 scans season 9's
        # three pairs, and every one of them has a video in rank 1's own block {4 .. 7})
        sent = {}
        for run in everything:
            scanned_by = next(r for r, g in enumerate(got) if g["pair_range"][0] <= run[0] < sum(g["pair_range"]))
            for owner in {v // block for v in pairs[run[0]]}:
                sent[scanned_by, owner] = sent.get((scanned_by, owner), 0) + 1
        assert max(sent.values()) > 4, sent
    union = set()
    for rank, g in enumerate(got):
        assert g["jobs"][0]["held"] == everything == g["jobs"][1]["held"]
        assert not g["jobs"][0]["form"]["directed_runs"] and not g["jobs"][1]["form"]["directed_runs"]
        job = g["jobs"][2]
        assert job["form"]["directed_runs"] is True
        first, count = g["video_block"]
        mine = [run for run in everything if any(first <= v < first + count for v in pairs[run[0]])]
        assert sorted(job["held"]) == sorted(mine), rank
        union.update(map(tuple, job["held"]))
        assert job["comm"]["scans_repeated"] == (1 if shard_epilogue == "directed-overflow" else 0)
    assert union == set(map(tuple, everything))
    assert any(len(g["jobs"][2]["held"]) < len(everything) for g in got)
