"""-m gpu: resident videos in the streaming all-pairs comparator (needle_hip_crossmatcher_new_resident): K known videos in
front of N arriving ones, only the pairs with an arriving end searched.  The checker is the oracle's table DP over the live
pairs, numbered over all V = K + N videos; runs are compared as sorted lists (src_end, dst_end, len, src_match_hash,
dst_match_hash) per problem, so a lost run, a doubled run, a run under the wrong problem or any run of a resident pair fails."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests.test_gpu_crossmatcher import (LENS, MIN_LENS, THRESHOLDS, by_pair, cuttings, dp, nonempty, one_item_per_feed, one_shot,
                                         pair_index, pairs_of, planted, rand_hashes)
from tests.test_gpu_crossmatcher_regions import MAX_ITEMS, MIN_LEN, season
from tests.test_gpu_crossmatcher_regions import cuttings as region_cuttings
from tests.test_gpu_scan_threshold import _dp_runs, _masks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def live_pairs(k, videos):
    return [(a, b) for a, b in pairs_of(videos) if b >= k]


def decode(problem, videos, regions=1):
    pair, r = divmod(problem, regions)
    return next((a, b, r) for a, b in pairs_of(videos) if pair_index(a, b, videos) == pair)


def oracle_live(rows, k, t, min_len, regions=1):
    """{problem: sorted runs} of the table DP over the live problems; rows[video * regions + region] over all videos."""
    videos = len(rows) // regions
    return nonempty({pair_index(a, b, videos) * regions + r: dp(rows[a * regions + r], rows[b * regions + r], t, min_len[r])
                     for a, b in live_pairs(k, videos) for r in range(regions)})


def live_cells(rows, k, regions=1):
    videos = len(rows) // regions
    return sum(max(len(rows[a * regions + r]) - 1, 0) * max(len(rows[b * regions + r]) - 1, 0)
               for a, b in live_pairs(k, videos) for r in range(regions))


def new(rows, k, max_items, min_len, t):
    regions = len(max_items)
    videos = len(rows) // regions - k
    m = capi.CrossMatcher.with_resident(rows[:k * regions], videos, max_items, min_len, t)
    assert m.resident == k and m.shape() == (videos, regions) and m.lanes == videos * regions
    return m


def arriving_only(schedule, first_lane):
    """A schedule over all rows cut down to the arriving lanes (feeds, and ("finish", lanes) steps)."""
    out = []
    for step in schedule:
        if step[0] == "finish":
            out.append(("finish", [x - first_lane for x in step[1] if x >= first_lane]))
        else:
            out.append(list(step[first_lane:]))
    return out


def stream(rows, k, schedule, t, max_items, min_len):
    """`schedule` over the arriving lanes.  Everything is fed, then what is left is finished: ({problem: sorted runs}, stats)."""
    regions = len(max_items)
    m = new(rows, k, max_items, min_len, t)
    lanes = rows[k * regions:]
    pos = [0] * len(lanes)
    for step in schedule:
        if step[0] == "finish":
            m.finish(step[1])
            continue
        chunks = []
        for q, part in enumerate(step):
            if part is None:
                chunks.append(None)
                continue
            assert part[0] == pos[q] and part[1] <= len(lanes[q])
            chunks.append(lanes[q][part[0]: part[1]])
            pos[q] = part[1]
        m.feed(chunks)
    assert pos == [len(x) for x in lanes] and [m.lane(q)[0] for q in range(len(lanes))] == pos
    m.finish()
    assert m.ready()[1] is True and all(m.lane(q)[1] for q in range(len(lanes)))
    return by_pair(m.runs()), m.stats()


def capacity(p, k):
    """The arriving lanes' capacity: 300 where B arrives; 40 for C and F against residents of 257 and 300."""
    return max(2, max(len(x) for x in p.lanes[k:]) + (3 if k == 4 else 0))


# ---- 1. every split of the planted season --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("min_len", MIN_LENS)
@pytest.mark.parametrize("t", THRESHOLDS)
def test_every_split_of_the_planted_season(t, min_len, k):
    p = planted(t, min_len)
    want = {prob: v for prob, v in p.oracle().items() if decode(prob, 6)[1] >= k}
    assert want == oracle_live(p.lanes, k, t, [min_len])
    cap = capacity(p, k)
    assert cap == {1: 300, 2: 300, 3: 300, 4: 40, 5: 2}[k]
    for name, schedule in cuttings(p):
        got, stats = stream(p.lanes, k, arriving_only(schedule, k), t, [cap], [min_len])
        assert got == want, (k, name)
        assert stats[2] == live_cells(p.lanes, k), (k, name)
    if k == 4 and t < 32:                                                        # (A, C) and (B, C) are there, (A, B) is not
        assert pair_index(1, 4, 6) in want and pair_index(3, 4, 6) in want and pair_index(1, 3, 6) in p.oracle()


# ---- 2. the same against the existing object -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 2, 3, 4, 5))
def test_the_plain_object_over_all_lanes_reports_the_same_live_runs(k):
    t, min_len = 10, 8
    p = planted(t, min_len)
    lens = [len(x) for x in p.lanes]
    plain = capi.CrossMatcher(6, 300, min_len, t)
    plain.feed([x if q < k and len(x) else None for q, x in enumerate(p.lanes)])  # the residents whole and finished first
    plain.finish(list(range(k)))
    schedule = arriving_only(one_item_per_feed(lens), k) if k >= 4 else arriving_only(list(cuttings(p))[-1][1], k)
    for feed in schedule:
        chunks = [None] * k
        for q, part in enumerate(feed):
            chunks.append(None if part is None else p.lanes[k + q][part[0]: part[1]])
        plain.feed(chunks)
    plain.finish()
    all_runs = by_pair(plain.runs())
    assert all_runs == p.oracle()
    want = {prob: v for prob, v in all_runs.items() if decode(prob, 6)[1] >= k}
    got, stats = stream(p.lanes, k, schedule, t, [capacity(p, k)], [min_len])
    assert got == want
    resident_cells = sum(max(lens[a] - 1, 0) * max(lens[b] - 1, 0) for a, b in pairs_of(k))
    assert stats[2] == live_cells(p.lanes, k) == plain.stats()[2] - resident_cells


# ---- 3. reported when the rule says so -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_len", MIN_LENS)
@pytest.mark.parametrize("t", THRESHOLDS)
def test_runs_are_reported_when_the_rule_says_so_with_residents(t, min_len):
    """The rule of the plain object with Ja = n_a for a resident from the first round on: after any feed a pair has reported
    exactly the runs of the prefixes' list with src_end < Ja - 1 and dst_end < Jb - 1.  A run into a resident's last row
    (src_end = n_a - 1) is therefore reported only in the round that finishes its lane."""
    k = 2                                                                        # D and A resident; E, B, C, F arrive
    p = planted(t, min_len)
    lens = [len(x) for x in p.lanes]
    m = new(p.lanes, k, [300], [min_len], t)
    fed = lens[:k] + [0] * (6 - k)
    before, closed = [], {}
    for feed in one_item_per_feed(lens[k:]):
        q = next(i for i, part in enumerate(feed) if part is not None)
        m.feed([None if part is None else p.lanes[k + i][part[0]: part[1]] for i, part in enumerate(feed)])
        fed[k + q] += 1
        assert m.lane(q) == (fed[k + q], False)
        raw = m.runs()
        now = [tuple(int(v) for v in x) for x in raw]
        assert now[:len(before)] == before, fed                                  # appended, never revised
        before = now
        for a, b in live_pairs(k, 6):                                            # (only this lane's pairs have changed)
            if k + q in (a, b):
                runs = dp(p.lanes[a][:fed[a]], p.lanes[b][:fed[b]], t, min_len)
                closed[pair_index(a, b, 6)] = [r for r in runs if r[0] < fed[a] - 1 and r[1] < fed[b] - 1]
        assert by_pair(raw) == nonempty(closed), fed
    ab = pair_index(1, 3, 6)
    last_row = [r for r in p.oracle()[ab] if r[0] == LENS[1] - 1]
    assert last_row and not any(r[0] == LENS[1] - 1 for r in by_pair(m.runs()).get(ab, []))   # planted "ends at i = n - 1": still held
    m.finish([0, 2, 3])                                                          # E, C, F: B's pairs with the residents stay open
    assert not any(r[0] == LENS[1] - 1 for r in by_pair(m.runs()).get(ab, []))
    m.finish([1])                                                                # B
    assert [r for r in by_pair(m.runs())[ab] if r[0] == LENS[1] - 1] == last_row
    assert m.ready()[1] and by_pair(m.runs()) == oracle_live(p.lanes, k, t, [min_len])
    assert [tuple(int(v) for v in x) for x in m.runs()][:len(before)] == before


# ---- 4. two regions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 4))
@pytest.mark.parametrize("t", THRESHOLDS)
def test_two_regions_with_residents(t, k):
    """The season of the regions test with videos 0 .. k - 1 resident in both regions: resident rows of 0, 120 (and, k = 4, 2
    and 90) hashes in region 1.  problem = pair * 2 + region over all six videos."""
    s = season(t)
    want = {prob: v for prob, v in s.oracle().items() if decode(prob, 6, 2)[1] >= k}
    assert want == oracle_live(s.lanes, k, t, MIN_LEN, 2)
    assert any(prob % 2 for prob in want) and any(prob % 2 == 0 for prob in want)
    caps = MAX_ITEMS if k == 2 else (40, 35)                                     # (k = 4: lanes of 37, 0 and 1, 33 against rows of 300 and 120)
    for name, schedule in region_cuttings(s):
        got, stats = stream(s.lanes, k, arriving_only(schedule, 2 * k), t, caps, MIN_LEN)
        assert got == want, (k, name)
        assert stats[2] == live_cells(s.lanes, k, 2), (k, name)


# ---- 5. fixed launches -----------------------------------------------------------------------------------------------------------
def test_launches_do_not_depend_on_the_residents_or_on_who_has_data():
    rng = np.random.default_rng(8)
    per_round = None
    for k in (1, 40):
        rows = [rand_hashes(rng, 20 + 3 * (q % 7)) for q in range(k)]
        m = capi.CrossMatcher.with_resident(rows, 3, [200], [3], 10)
        chunk = rand_hashes(rng, 6)
        for step in range(10):
            was = m.stats()
            m.feed([chunk if (step + lane) % 2 else None for lane in range(3)])
            now = m.stats()
            per_round = per_round or now[1] - was[1]
            assert now[1] - was[1] == per_round == 3, (k, step)
            assert now[3] == was[3] >= capi.CrossMatcher.state_bytes(3, [200], [len(x) for x in rows])
        was = m.stats()
        m.feed([chunk, None, None])                                              # one lane alone
        assert m.stats()[1] - was[1] == per_round
        was = m.stats()
        m.feed([None, None, None])                                               # nothing: no round
        assert m.stats() == was
        m.finish([0])                                                            # a round without data adds no cells
        assert m.stats()[1] - was[1] == per_round and m.stats()[2] == was[2]
        m.finish()
        fed = [m.lane(q)[0] for q in range(3)]
        resident_rows = sum(len(x) - 1 for x in rows)
        assert m.stats()[2] == resident_rows * sum(f - 1 for f in fed) + sum((fed[a] - 1) * (fed[b] - 1) for a, b in pairs_of(3))


# ---- 6. sizes the small tables miss ------------------------------------------------------------------------------------------------
def test_a_resident_of_several_carried_workgroups_and_a_feed_of_several_pieces():
    """A resident of 2 300 hashes takes three workgroups of carried rows; the arriving lane is fed 700 items in one feed, cut
    into pieces of 512.  Copies cross rows 1 024 and 2 048, one crosses the piece boundary, one runs into the last row."""
    rng = np.random.default_rng(31)
    long_row, other = rand_hashes(rng, 2300), rand_hashes(rng, 90)
    lane, second = rand_hashes(rng, 700), rand_hashes(rng, 300)
    copies = ((0, 2, 1000, 100, 60), (0, 2, 2010, 300, 80), (0, 2, 1500, 490, 50), (0, 2, 2260, 600, 40), (0, 2, 1, 650, 50),
              (1, 2, 10, 560, 30), (0, 3, 2040, 20, 20), (2, 3, 500, 100, 40))
    rows = [long_row, other, lane, second]
    for a, b, ra, cb, length in copies:
        rows[b][cb: cb + length] = rows[a][ra: ra + length] ^ _masks([2] * length, rng, 0)
    t, min_len = 9, 12
    want = oracle_live(rows, 2, t, [min_len])
    for a, b, ra, cb, length in copies:                                          # (the background may lengthen a copy)
        assert any(r[:2] == (ra + length - 1, cb + length - 1) and r[2] >= length for r in want[pair_index(a, b, 4)]), (a, b, ra, cb)
    assert any(r[0] == 2299 for r in want[pair_index(0, 2, 4)])
    for schedule in ([[(0, 700), (0, 300)]], [[(0, 700), None], [None, (0, 300)]], [[(0, 3), (0, 300)], [(3, 700), None]]):
        got, stats = stream(rows, 2, schedule, t, [800], [min_len])
        assert got == want, schedule
        assert stats[2] == live_cells(rows, 2)


def test_a_resident_of_65540_hashes_makes_the_whole_state_32_bit():
    rng = np.random.default_rng(22)
    long_row = rand_hashes(rng, 65540)
    lane, second = rand_hashes(rng, 48), rand_hashes(rng, 40)
    lane[5:45] = long_row[65500:65540] ^ _masks([1] * 40, rng, 0)                # a run into row 65 539
    second[10:30] = lane[20:40] ^ _masks([1] * 20, rng, 0)
    rows = [long_row, lane, second]
    want = oracle_live(rows, 1, 9, [5])
    assert any(r[:2] == (65539, 44) and r[2] >= 40 for r in want[pair_index(0, 1, 3)]) and pair_index(1, 2, 3) in want
    # 32-bit entries although the lanes hold 48: one pair's L frontier, two histories, two col frontiers, the resident hashes
    assert capi.CrossMatcher.state_bytes(2, [48], [65540]) == 1 * 4 * 48 * 4 + 2 * 48 * 4 + 2 * 2 * 65540 * 4 + 65540 * 4
    assert capi.CrossMatcher.state_bytes(2, [48], [65535]) == 1 * 4 * 48 * 2 + 2 * 48 * 4 + 2 * 2 * 65535 * 2 + 65535 * 4
    got, stats = stream(rows, 1, [[(0, 20), None], [(20, 21), (0, 40)], [(21, 48), None]], 9, [48], [5])
    assert got == want
    assert stats[2] == live_cells(rows, 1) and stats[3] >= capi.CrossMatcher.state_bytes(2, [48], [65540])


# ---- 7. slab overflow --------------------------------------------------------------------------------------------------------------
_SLAB_CHILD = """
import json, sys
import numpy as np
from needle_amd import capi
from tests.test_gpu_crossmatcher import by_pair
rows = [np.full(64, 0x5A5A5A5A, dtype=np.uint32) for _ in range(4)]
m = capi.CrossMatcher.with_resident(rows[:2], 2, [64], [8], 10)
for a in range(0, 64, 16):
    m.feed([x[a:a + 16] for x in rows[2:]])
m.finish()
print(json.dumps({"runs": {str(k): v for k, v in by_pair(m.runs()).items()}, "stats": m.stats()}))
"""


def _slab_child(slab):
    env = {k: v for k, v in os.environ.items() if k != "NEEDLE_HIP_CROSSMATCHER_RUN_SLAB"}
    if slab:
        env["NEEDLE_HIP_CROSSMATCHER_RUN_SLAB"] = str(slab)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", _SLAB_CHILD], cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True, timeout=120, check=True)
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_a_slab_too_small_loses_nothing_with_residents():
    src = np.full(64, 0x5A5A5A5A, dtype=np.uint32)
    want = _dp_runs(src, src, 10, 8)
    assert len(want) > 100
    small, roomy = _slab_child(4), _slab_child(0)
    live = sorted(str(pair_index(a, b, 4)) for a, b in live_pairs(2, 4))
    assert len(live) == 5 and str(pair_index(0, 1, 4)) not in live
    for child in (small, roomy):
        assert sorted(child["runs"]) == live
        for runs in child["runs"].values():
            assert [tuple(r) for r in runs] == want
    assert small["stats"][1] > roomy["stats"][1]                                 # the repeated rounds
    assert small["stats"][0] == roomy["stats"][0] == 4


# ---- 8. from a feeder, to results --------------------------------------------------------------------------------------------------
def _results(res):
    return [None if r is None else (r.opening, r.ending) for r in res]


def _from_a_feeder_to_results_with_residents():
    seconds = (60.0, 75.0, 90.0, 70.0)
    pcms = [synth.make_episode(k, s, 20.0).pcm for k, s in enumerate(seconds)]   # every episode holds the same 20 s intro
    k, n, t, min_len = 2, 2, 10, 30
    items = capi.fingerprint(pcms, 1, 2)
    want = {prob: v for prob, v in one_shot(items, t, min_len).items() if decode(prob, 4)[1] >= k}
    assert sorted(want) == sorted(pair_index(a, b, 4) for a, b in live_pairs(k, 4))
    assert min(max(r[2] for r in runs) for runs in want.values()) >= 60          # 20 s: ~80 kept items
    hd = O.duration_from_secs_f32(0.3)
    resident = []
    for x in items[:k]:                                                          # the library's records of the known videos
        ts = [ts for _, ts in O.step_and_timestamp(np.zeros(2 * len(x), dtype=np.uint32), hd)][:len(x)]
        resident.append(capi.FrameHashes.new(list(zip(x.tolist(), ts)), (), hd, ""))
    f = capi.Feeder(n, 1, 11025, capi.SAMPLE_S16, 2)
    m = capi.CrossMatcher.with_resident([fh.opening_data()[0] for fh in resident], n, [max(len(x) for x in items[k:])], [min_len], t)
    half = 11025 // 2
    pos = [0] * n
    step, early = 0, 0
    while not m.ready()[1]:
        chunk = []
        for q in range(n):
            take = 0 if (step + q) % 3 == 0 else half                            # the lanes out of step
            chunk.append(pcms[k + q][pos[q]: pos[q] + take] if take and pos[q] < len(pcms[k + q]) else None)
            pos[q] = min(len(pcms[k + q]), pos[q] + take)
        f.feed(chunk)
        ended = [q for q in range(n) if pos[q] == len(pcms[k + q]) and not f.ready(q)[2]]
        if ended:
            f.finish(ended)
        m.feed_from_feeder(f)
        assert [m.lane(q) for q in range(n)] == [(f.ready(q)[0], f.ready(q)[2]) for q in range(n)]
        if not any(m.lane(q)[1] for q in range(n)):                              # no lane finished: against a resident too
            early = max(early, max((int(x["len"]) for x in m.runs() if decode(int(x["problem"]), 4)[0] < k), default=0))
        step += 1
    assert early >= 60, "a shared segment's run against a resident is reported before the lane finishes"
    assert [m.lane(q) for q in range(n)] == [(len(x), True) for x in items[k:]]
    runs = m.runs()
    assert by_pair(runs) == want
    m.feed_from_feeder(f)                                                        # nothing new: nothing happens
    assert by_pair(m.runs()) == want
    fhs = resident + [f.frame_hashes(q) for q in range(n)]
    cmp = capi.Comparator([f"ep{v}.wav" for v in range(4)], min_opening_duration=10)
    got, ref = _results(cmp.results_from_runs(fhs, runs, first_video=k)), _results(cmp.run_with_frame_hashes(fhs))
    assert got[k:] == ref[k:]
    assert all(r is not None and r[0] is not None for r in ref[k:])


def test_from_a_feeder_to_results_with_residents():
    _from_a_feeder_to_results_with_residents()


def test_from_a_feeder_to_results_with_residents_f64(monkeypatch):
    monkeypatch.setenv("NEEDLE_HIP_STFT", "f64")
    _from_a_feeder_to_results_with_residents()


# ---- 9. existing paths -------------------------------------------------------------------------------------------------------------
def test_objects_without_residents_are_what_they_were():
    m = capi.CrossMatcher(5, 100, 4, 10)
    assert m.resident == 0 and m.shape() == (5, 1)
    assert m.stats()[3] >= capi.CrossMatcher.state_bytes(5, 100) == 10 * 4 * 100 * 2 + 5 * 100 * 4
    r = capi.CrossMatcher.with_regions(5, (100, 60), (4, 3), 10)
    assert r.resident == 0 and r.shape() == (5, 2)
    assert capi.CrossMatcher.state_bytes(5, (100, 60)) == capi.CrossMatcher.state_bytes(5, (100, 60), []) == 10 * 4 * 160 * 2 + 5 * 160 * 4
    slab = 32 + 4096 * 24
    assert m.stats()[3] == capi.CrossMatcher.state_bytes(5, 100) + slab and r.stats()[3] == capi.CrossMatcher.state_bytes(5, (100, 60)) + slab
