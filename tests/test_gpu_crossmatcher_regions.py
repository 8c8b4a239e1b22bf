"""-m gpu: openings and endings in one streaming all-pairs comparator (needle_hip_crossmatcher_new_regions).  The lanes are
videos x 2, lane = video * 2 + region, and only lanes of one region are matched.  The checker for every run list is the
oracle's table DP per (pair, region), as tests/test_gpu_crossmatcher.py uses it, and next to it capi.hamming_runs over the
same problems numbered pair * 2 + region; runs are compared as sorted lists (src_end, dst_end, len, src_match_hash,
dst_match_hash) per problem: exact equality, so a run lost, reported twice or reported under another problem fails."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from needle_amd import capi, synth
from tests.test_gpu_crossmatcher import (LENS, by_pair, chunks_from_cuts, dp, nonempty, one_item_per_feed, pair_index, pairs_of,
                                         planted, rand_hashes)
from tests.test_gpu_library_rates import windows
from tests.test_gpu_scan_threshold import _dp_runs, _masks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

THRESHOLDS = (0, 10, 32)
R = 2
MAX_ITEMS, MIN_LEN = (300, 120), (8, 5)
INVALID = capi.ERROR_NAMES.index("InvalidArgument")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def problem_index(a, b, r, videos, regions=R):
    return pair_index(a, b, videos) * regions + r


def oracle(lanes, videos, t, min_len, regions=R):
    """{problem: sorted runs} of the table DP per (pair, region); lanes[video * regions + region]."""
    return nonempty({problem_index(a, b, r, videos, regions): dp(lanes[a * regions + r], lanes[b * regions + r], t, min_len[r])
                     for a, b in pairs_of(videos) for r in range(regions)})


def one_shot(lanes, videos, t, min_len, regions=R):
    """capi.hamming_runs over the same problems (those of two lanes that hold anything): {problem: sorted runs}."""
    some = [(a, b, r) for a, b in pairs_of(videos) for r in range(regions) if len(lanes[a * regions + r]) and len(lanes[b * regions + r])]
    got = by_pair(capi.hamming_runs(list(lanes), [(a * regions + r, b * regions + r, min_len[r]) for a, b, r in some], t))
    return {problem_index(*some[k], videos, regions): v for k, v in got.items()}


def new(videos, max_items, min_len, t):
    m = capi.CrossMatcher.with_regions(videos, max_items, min_len, t)
    assert m.shape() == (videos, len(max_items)) and m.lanes == videos * len(max_items)
    return m


def stream(lanes, schedule, t, max_items, min_len):
    """`schedule`: steps, each a feed (a list with one (first, end) slice or None per lane) or ("finish", lanes).  Everything
    is fed, then what is left is finished: ({problem: sorted runs}, stats)."""
    n = len(lanes)
    m = new(n // len(max_items), max_items, min_len, t)
    pos = [0] * n
    for step in schedule:
        if step[0] == "finish":
            m.finish(step[1])
            continue
        chunks = []
        for k, part in enumerate(step):
            if part is None:
                chunks.append(None)
                continue
            assert part[0] == pos[k] and part[1] <= len(lanes[k])
            chunks.append(lanes[k][part[0]: part[1]])
            pos[k] = part[1]
        m.feed(chunks)
    assert pos == [len(x) for x in lanes] and [m.lane(k)[0] for k in range(n)] == pos
    m.finish()
    assert m.ready()[1] is True and all(m.lane(k)[1] for k in range(n))
    return by_pair(m.runs()), m.stats()


# ---- the planted season, two regions ------------------------------------------------------------------------------------------
E_LENS = (0, 120, 2, 90, 1, 33)                  # region 1's lanes, by video


class Endings:
    """Region 1 of the planted season: videos of 0, 120, 2, 90, 1 and 33 hashes on a random background.  In the table of
    videos (1, 3) -- 120 rows, 90 columns -- stretches of video 1 are copied into video 3 at distance exactly min(t, 32), fenced
    by a cell at t + 1: from
    column 1, from row 1, exactly min_len and one short of it, into the last row and into the last column.  Video 5 is video
    3's last 33 items: pair (3, 5) is one run into the corner (last row and last column at once), and pair (1, 5) ends with
    (1, 3)'s run into the last column.  Video 2's two items lie at distance t from two of video 1's."""

    def __init__(self, t, min_len, seed=3):
        rng = np.random.default_rng(seed * 104729 + t * 101 + min_len)
        n, M, T = E_LENS[1], E_LENS[3], min(t, 32)
        big, dst = rand_hashes(rng, n), rand_hashes(rng, M)
        L = min_len + 2
        self.cuts = {k: set() for k in range(6)}
        self.placed = {}

        def put(name, a, b, length):
            dst[b: b + length] = big[a: a + length] ^ _masks([T] * length, rng, a)
            for i, j in ((a - 1, b - 1), (a + length, b + length)):               # fenced by a cell at t + 1 at both ends
                if t < 32 and 0 <= i < n and 0 <= j < M:
                    dst[j] = big[i] ^ _masks([t + 1], rng, i)[0]
            self.cuts[1] |= {a, a + 1, a + length - 1, a + length}
            self.cuts[3] |= {b, b + 1, b + length - 1, b + length}
            self.placed[name] = (a + length - 1, b + length - 1, length)
        put("from column 1", 10, 1, L)
        put("from row 1", 1, 12, L)
        put("exactly min_len", 40, 25, min_len)
        put("min_len - 1", 60, 40, min_len - 1)
        put("into the last row", n - L, 50, L)
        put("into the last column", 70, M - L, L)
        tail = M - E_LENS[5]
        self.cuts[5] = {c - tail for c in self.cuts[3]}
        small = np.array([big[30], big[31]], dtype=np.uint32) ^ _masks([T, T], rng, 0)
        self.lanes = [np.zeros(0, dtype=np.uint32), big, small, dst, rand_hashes(rng, 1), dst[tail:].copy()]
        assert tuple(len(x) for x in self.lanes) == E_LENS
        self.cuts = {k: {c for c in v if 0 < c < E_LENS[k]} for k, v in self.cuts.items()}


class Season:
    """Both regions: lanes[2 v] is the existing planted season's lane v, lanes[2 v + 1] the Endings table's."""

    def __init__(self, t):
        self.t = t
        self.opening = planted(t, MIN_LEN[0])
        self.ending = Endings(t, MIN_LEN[1])
        self.lanes, self.cuts = [], []
        for v in range(6):
            self.lanes += [self.opening.lanes[v], self.ending.lanes[v]]
            self.cuts += [self.opening.cuts[v], self.ending.cuts[v]]
        self.lens = [len(x) for x in self.lanes]
        assert self.lens[0::2] == [LENS[v] for v in range(6)] == [2, 257, 1, 300, 37, 0] and tuple(self.lens[1::2]) == E_LENS
        self._oracle = None

    def oracle(self):
        if self._oracle is None:
            self._oracle = oracle(self.lanes, 6, self.t, MIN_LEN)
            even = {k // 2: v for k, v in self._oracle.items() if k % 2 == 0}
            assert even == self.opening.oracle()                                 # region 0 is the existing season's list
            e, n, M = self.ending, E_LENS[1], E_LENS[3]
            p13, p15, p35 = (problem_index(a, b, 1, 6) for a, b in ((1, 3), (1, 5), (3, 5)))
            ends = {name: [r for r in self._oracle[p13] if r[:2] == at[:2] and r[2] >= at[2]] for name, at in e.placed.items()}
            for name in ("from column 1", "from row 1", "exactly min_len") if self.t < 32 else ():     # what was planted is there
                assert ends[name], name
            for name in ("into the last row", "into the last column"):
                assert ends[name], name
            assert e.placed["into the last row"][0] == n - 1 and e.placed["into the last column"][1] == M - 1
            assert any(r[1] == E_LENS[5] - 1 and r[0] < n - 1 for r in self._oracle[p15])           # into the last column
            assert any(r[:3] == (M - 1, E_LENS[5] - 1, E_LENS[5] - 1) for r in self._oracle[p35])   # into the corner
        return self._oracle


_SEASONS = {}


def season(t):
    if t not in _SEASONS:
        _SEASONS[t] = Season(t)
    return _SEASONS[t]


def out_of_step(per_lane_chunks, rng, share=(0.7, 0.3)):
    """Every lane's chunks in order; a feed serves a lane of region r with probability share[r], so the regions drift apart;
    some feeds are empty."""
    left = [list(c) for c in per_lane_chunks]
    out = []
    while any(left):
        if rng.random() < 0.05:
            out.append([None] * len(left))
            continue
        out.append([c.pop(0) if c and rng.random() < share[k % R] else None for k, c in enumerate(left)])
    return out


def cuttings(s):
    lens = s.lens
    n = len(lens)
    yield "one item per feed, the lanes alternating", one_item_per_feed(lens)
    yield "whole lanes in one feed", [[(0, x) if x else None for x in lens]]
    for seed in range(3):
        rng = np.random.default_rng(300 + seed)
        per_lane = []
        for k, x in enumerate(lens):
            extra = set(rng.choice(np.arange(1, x), size=int(rng.integers(1, min(20, x))), replace=False).tolist()) if x > 2 else set()
            per_lane.append(chunks_from_cuts(s.cuts[k] | extra, x))
        yield f"random cuts, the regions out of step {seed}", out_of_step(per_lane, rng, ((0.7, 0.3), (0.3, 0.7), (0.5, 0.5))[seed])
    ending_lanes = list(range(1, n, 2))
    first = [[(0, lens[q]) if q == k and lens[q] else None for q in range(n)] for k in ending_lanes]
    rng = np.random.default_rng(77)
    per_lane = [chunks_from_cuts(s.cuts[k], x) if k % 2 == 0 else [] for k, x in enumerate(lens)]
    yield "region 1 fed and finished before region 0 starts", first + [("finish", ending_lanes)] + out_of_step(per_lane, rng, (0.6, 0.0))


# ---- 1. any cutting, two regions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", THRESHOLDS)
def test_any_cutting_of_two_regions_equals_the_one_shot_and_the_oracle(t):
    s = season(t)
    want = s.oracle()
    assert any(k % 2 for k in want) and any(k % 2 == 0 for k in want)
    assert one_shot(s.lanes, 6, t, MIN_LEN) == want
    for name, schedule in cuttings(s):
        got, _ = stream(s.lanes, schedule, t, MAX_ITEMS, MIN_LEN)
        assert got == want, name


# ---- 2. regions do not see each other -----------------------------------------------------------------------------------------
def test_regions_do_not_see_each_other():
    """Video 0's opening and video 1's ending hold the same 60 hashes, and so do video 2's opening and its ending: a matcher
    over six lanes without regions would report both.  Two real copies inside a region are found."""
    rng = np.random.default_rng(31)
    t, min_len = 10, (8, 8)
    lanes = [rand_hashes(rng, x) for x in (100, 80, 100, 80, 100, 80)]           # lane = video * 2 + region
    shared, own = rand_hashes(rng, 60), rand_hashes(rng, 60)
    lanes[0][20:80] = shared
    lanes[3][10:70] = shared
    lanes[4][30:90] = own
    lanes[5][5:65] = own
    lanes[2][3:33] = lanes[0][40:70] ^ _masks([2] * 30, rng, 0)                  # region 0, videos (0, 1)
    lanes[5][66:80] = lanes[1][20:34] ^ _masks([2] * 14, rng, 0)                 # region 1, videos (0, 2), into the last column
    assert max(r[2] for r in _dp_runs(lanes[0], lanes[3], t, 8)) >= 59 and max(r[2] for r in _dp_runs(lanes[4], lanes[5], t, 8)) >= 59
    want = oracle(lanes, 3, t, min_len)
    assert sorted(want) == [problem_index(0, 1, 0, 3), problem_index(0, 2, 1, 3)]
    assert all(r[2] < 40 for runs in want.values() for r in runs)
    assert one_shot(lanes, 3, t, min_len) == want
    whole = [(0, len(x)) for x in lanes]
    by_item = one_item_per_feed([len(x) for x in lanes])
    for schedule in ([whole], by_item):
        got, _ = stream(lanes, schedule, t, (100, 80), min_len)
        assert got == want


# ---- 3. completion is per region ----------------------------------------------------------------------------------------------
def test_completion_is_per_region():
    t = 10
    s = season(t)
    want = s.oracle()
    m = new(6, MAX_ITEMS, MIN_LEN, t)
    m.feed([x if len(x) else None for x in s.lanes])
    m.finish([1, 3, 5])                                                          # some of region 1: nothing of it is complete ...
    m.finish([7, 9, 11])                                                         # ... now all of it, and nothing of region 0
    assert [m.lane(k) for k in range(12)] == [(s.lens[k], bool(k % 2)) for k in range(12)]
    got = by_pair(m.runs())
    assert {k: v for k, v in got.items() if k % 2} == {k: v for k, v in want.items() if k % 2}     # final, and the oracle's
    closed = {}
    for a, b in pairs_of(6):                                                     # an even problem: only what a cell has broken
        na, nb = s.lens[2 * a], s.lens[2 * b]
        closed[problem_index(a, b, 0, 6)] = [r for r in want.get(problem_index(a, b, 0, 6), []) if r[0] < na - 1 and r[1] < nb - 1]
        assert all(r[0] < na - 1 and r[1] < nb - 1 for r in got.get(problem_index(a, b, 0, 6), []))
    assert {k: v for k, v in got.items() if k % 2 == 0} == nonempty(closed)
    assert nonempty(closed) != {k: v for k, v in want.items() if k % 2 == 0}     # (something of region 0 is still open)
    assert m.ready()[1] is False
    before = [tuple(int(v) for v in x) for x in m.runs()]
    m.finish()
    assert m.ready()[1] is True and by_pair(m.runs()) == want
    assert [tuple(int(v) for v in x) for x in m.runs()][:len(before)] == before  # appended, never revised


# ---- 4. every cell once, fixed launches ---------------------------------------------------------------------------------------
def test_every_cell_once_and_fixed_launches():
    rng = np.random.default_rng(8)
    chunk = rand_hashes(rng, 6)
    single = capi.CrossMatcher(3, 200, 3, 10)
    single.feed([chunk, None, chunk])
    per_round = single.stats()[1]
    assert per_round >= 1 and single.shape() == (3, 1)
    for videos in (3, 12):
        for regions in (1, 2):
            max_items, min_len = (200, 100)[:regions], (3, 2)[:regions]
            n = videos * regions
            m = new(videos, max_items, min_len, 10)
            state, fed = [], [0] * n
            for k in range(30):
                was = m.stats()[1]
                feed = [chunk if (k + lane) % 2 else None for lane in range(n)]   # only the lanes with data differ
                m.feed(feed)
                fed = [x + (0 if c is None else len(c)) for x, c in zip(fed, feed)]
                assert m.stats()[1] - was == per_round, (videos, regions, k)
                state.append(m.stats()[3])
            for region in range(regions):                                        # one region's lanes alone carry data
                was = m.stats()[1]
                feed = [chunk if lane % regions == region else None for lane in range(n)]
                m.feed(feed)
                fed = [x + (0 if c is None else len(c)) for x, c in zip(fed, feed)]
                assert m.stats()[1] - was == per_round, (videos, regions, region)
                state.append(m.stats()[3])
            was = m.stats()[1]
            m.finish(list(range(regions - 1, n, regions)))                       # the last region's lanes, then the rest
            m.finish()
            assert m.stats()[1] - was == (2 if regions == 2 else 1) * per_round and m.stats()[0] == 30 + regions
            assert [m.lane(k) for k in range(n)] == [(x, True) for x in fed]
            cells = sum((fed[a * regions + r] - 1) * (fed[b * regions + r] - 1) for a, b in pairs_of(videos) for r in range(regions))
            assert m.stats()[2] == cells                                         # the sum over the regions
            state.append(m.stats()[3])
            assert len(set(state)) == 1 and state[0] >= capi.CrossMatcher.state_bytes(videos, max_items)


# ---- 5. slab overflow ---------------------------------------------------------------------------------------------------------
_SLAB_CHILD = """
import json, sys
import numpy as np
from needle_amd import capi
from tests.test_gpu_crossmatcher import by_pair
lanes = [np.full(64 if k % 2 == 0 else 40, 0x5A5A5A5A, dtype=np.uint32) for k in range(6)]
m = capi.CrossMatcher.with_regions(3, (64, 40), (8, 5), 10)
for a in range(0, 64, 16):
    m.feed([x[a:a + 16] for x in lanes])
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


def test_a_slab_too_small_loses_nothing_in_either_region():
    want = []
    for items, min_len in ((64, 8), (40, 5)):
        src = np.full(items, 0x5A5A5A5A, dtype=np.uint32)
        want.append(_dp_runs(src, src, 10, min_len))
        assert len(want[-1]) > 60                                                # every diagonal of min_len cells or more is a run
    small, roomy = _slab_child(4), _slab_child(0)
    for child in (small, roomy):
        assert sorted(child["runs"], key=int) == ["0", "1", "2", "3", "4", "5"]
        for problem, runs in child["runs"].items():
            assert [tuple(r) for r in runs] == want[int(problem) % 2], problem    # nothing lost, nothing twice
    assert small["stats"][1] > roomy["stats"][1]                                 # the repeated rounds
    assert small["stats"][0] == roomy["stats"][0] == 4
    assert "NEEDLE_HIP_CROSSMATCHER_RUN_SLAB" not in os.environ


# ---- 6. pieces ----------------------------------------------------------------------------------------------------------------
def test_one_feed_wider_than_a_piece_in_both_regions():
    """One feed carries region-0 lanes of 700 / 1300 / 600 items and region-1 lanes of 300 / 40 / 513: it is cut into pieces
    of 512 items per lane, and copies cross the 512 boundaries of both sides in both regions."""
    rng = np.random.default_rng(25)
    sizes = (700, 300, 1300, 40, 600, 513)
    lanes = [rand_hashes(rng, x) for x in sizes]
    copies = ((0, 2, 480, 480, 80), (0, 2, 500, 1012, 40), (0, 2, 512 - 30, 600, 30), (0, 2, 512, 640, 30), (0, 4, 490, 490, 50),
              (2, 4, 1000, 440, 40), (2, 4, 1250, 550, 50),                      # region 0 (lanes 0, 2, 4)
              (1, 5, 200, 440, 30), (1, 3, 100, 8, 30), (3, 5, 5, 478, 35))      # region 1 (lanes 1, 3, 5): the last into the corner
    for a, b, ra, cb, L in copies:
        lanes[b][cb: cb + L] = lanes[a][ra: ra + L] ^ _masks([2] * L, rng, 0)
    t, min_len = 9, (12, 12)
    want = oracle(lanes, 3, t, min_len)
    for a, b, ra, cb, L in copies:                                               # (the background may lengthen a copy)
        assert a % 2 == b % 2
        assert any(r[:2] == (ra + L - 1, cb + L - 1) and r[2] >= L for r in want[problem_index(a // 2, b // 2, a % 2, 3)]), (a, b, ra, cb)
    assert one_shot(lanes, 3, t, min_len) == want
    got, stats = stream(lanes, [[(0, x) for x in sizes]], t, (1300, 513), min_len)
    assert got == want
    per_round = stats[1] // 4                                                    # pieces of 512: three rounds, and the finish
    assert stats[0] == 1 and stats[1] == 4 * per_round
    assert stats[2] == sum((sizes[2 * a + r] - 1) * (sizes[2 * b + r] - 1) for a, b in pairs_of(3) for r in range(R))
    got, _ = stream(lanes, [[(0, 700), None, None, (0, 40), None, (0, 3)], [None, (0, 300), (0, 1300), None, (0, 600), (3, 513)]],
                    t, (1300, 513), min_len)
    assert got == want


# ---- 7. wide state ------------------------------------------------------------------------------------------------------------
def test_a_region_of_65540_items_makes_the_whole_state_32_bit():
    rng = np.random.default_rng(24)
    long_lane = rand_hashes(rng, 65540)
    before, after = rand_hashes(rng, 48), rand_hashes(rng, 48)
    long_lane[65520:65540] = before[10:30] ^ _masks([1] * 20, rng, 0)            # a run into column 65 539 of (0, 1), region 1
    after[5:45] = long_lane[65500:65540] ^ _masks([1] * 40, rng, 0)              # ... and one into row 65 539 of (1, 2), region 1
    small = [rand_hashes(rng, x) for x in (48, 30, 40)]
    small[2][15:40] = small[0][20:45] ^ _masks([1] * 25, rng, 0)                 # a run in region 0, into (0, 2)'s last column
    lanes = [small[0], before, small[1], long_lane, small[2], after]
    max_items, min_len = (48, 65540), (5, 5)
    want = oracle(lanes, 3, 9, min_len)
    assert any(r[:2] == (65539, 44) and r[2] >= 40 for r in want[problem_index(1, 2, 1, 3)])
    assert any(r[:2] == (29, 65539) and r[2] >= 20 for r in want[problem_index(0, 1, 1, 3)])
    assert any(r[:2] == (44, 39) and r[2] >= 25 for r in want[problem_index(0, 2, 0, 3)])
    assert one_shot(lanes, 3, 9, min_len) == want
    assert capi.CrossMatcher.state_bytes(3, max_items) == 3 * 4 * (48 + 65540) * 4 + 3 * (48 + 65540) * 4
    schedule = [[(0, 20), (0, 20), None, (0, 30000), (0, 40), None], [(20, 48), (20, 21), (0, 30), (30000, 65540), None, (0, 48)],
                [None, (21, 48), None, None, None, None]]
    got, stats = stream(lanes, schedule, 9, max_items, min_len)
    assert got == want
    assert stats[2] == sum((len(lanes[2 * a + r]) - 1) * (len(lanes[2 * b + r]) - 1) for a, b in pairs_of(3) for r in range(R))
    assert stats[3] >= capi.CrossMatcher.state_bytes(3, max_items)


# ---- 8. from a feeder, to results with endings --------------------------------------------------------------------------------
def _results(res):
    return [None if r is None else (r.opening, r.ending) for r in res]


def _from_a_feeder_to_results_with_endings():
    seconds = (80.0, 90.0, 100.0, 88.0)
    pcms = [synth.make_episode(k, s, 20.0, 15.0).pcm for k, s in enumerate(seconds)]   # a shared 20 s intro and a shared 15 s outro
    videos, t, min_len = len(pcms), 10, (30, 25)
    streams, seeks = [], []
    for p in pcms:                                                               # lane 2k: the opening window; 2k + 1: from the ending seek point on
        (o0, on), (e0, en, seek) = windows(len(p), 1, 11025)
        streams += [p[o0: o0 + on], p[e0: e0 + en]]
        seeks.append(seek)
    n = 2 * videos
    f = capi.Feeder(n, 1, 11025, capi.SAMPLE_S16, 2)
    m = None
    half = 11025 // 2
    pos = [0] * n
    step, early = 0, [0, 0]
    while m is None or not m.ready()[1]:
        chunk = []
        for k in range(n):
            take = 0 if (step + k) % 3 == 0 else half                            # the lanes out of step
            chunk.append(streams[k][pos[k]: pos[k] + take] if take and pos[k] < len(streams[k]) else None)
            pos[k] = min(len(streams[k]), pos[k] + take)
        f.feed(chunk)
        ended = [k for k in range(n) if pos[k] == len(streams[k]) and not f.ready(k)[2]]
        if ended:
            f.finish(ended)
        if m is None:                                                            # capacities: what the windows will hold
            cap = [max(capi.feeder_num_ready(len(streams[k]), 11025, 1, 2, True) for k in range(r, n, 2)) for r in range(R)]
            m = new(videos, cap, min_len, t)
        last = all(f.ready(k)[2] for k in range(n))
        m.feed_from_feeder(f)
        assert [m.lane(k) for k in range(n)] == [(f.ready(k)[0], f.ready(k)[2]) for k in range(n)]
        if not last:
            assert not m.ready()[1]
            for x in m.runs():
                early[int(x["problem"]) % 2] = max(early[int(x["problem"]) % 2], int(x["len"]))
        step += 1
    items = [f.items(k) for k in range(n)]
    assert [m.lane(k) for k in range(n)] == [(len(x), True) for x in items]
    want = one_shot(items, videos, t, min_len)
    assert sorted(want) == list(range(12))                                       # every pair, both regions
    # the ending lanes end long before the opening lanes: region 1 was complete, and its longest run reported, before the last
    # round; of region 0 a shared intro's run was reported as soon as both lanes had passed it
    assert early[1] == max(r[2] for k, runs in want.items() if k % 2 for r in runs) >= min_len[1]
    assert early[0] >= 60, "a shared segment's run is reported before the last lane finishes"
    runs = m.runs()
    assert by_pair(runs) == want
    m.feed_from_feeder(f)                                                        # nothing new: nothing happens
    assert by_pair(m.runs()) == want
    with pytest.raises(capi.NeedleError) as e:                                   # lane for lane: a feeder of `videos` lanes is refused
        m.feed_from_feeder(capi.Feeder(videos, 1, 11025, capi.SAMPLE_S16, 2))
    assert e.value.code == INVALID
    fhs = [f.frame_hashes(2 * k, 2 * k + 1, seeks[k]) for k in range(videos)]
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(videos)], include_endings=True, min_opening_duration=10, min_ending_duration=10)
    got, ref = _results(cmp.results_from_runs(fhs, runs)), _results(cmp.run_with_frame_hashes(fhs))
    assert got == ref
    assert all(r is not None and r[0] is not None and r[1] is not None for r in ref)


def test_from_a_feeder_to_results_with_endings():
    _from_a_feeder_to_results_with_endings()


def test_from_a_feeder_to_results_with_endings_f64(monkeypatch):
    monkeypatch.setenv("NEEDLE_HIP_STFT", "f64")
    _from_a_feeder_to_results_with_endings()


# ---- the errors that need an object -------------------------------------------------------------------------------------------
def test_a_refused_call_moves_no_lane():
    rng = np.random.default_rng(9)
    m = new(3, (10, 4), (2, 2), 10)
    ok = [rand_hashes(rng, 3)] * 6
    m.feed(ok)
    state = ([m.lane(k) for k in range(6)], m.stats(), m.ready())
    for feed in ([rand_hashes(rng, 2), rand_hashes(rng, 2), None, None, None, None],       # lane 1 is region 1: capacity 4
                 [rand_hashes(rng, 7), None, None, None, rand_hashes(rng, 8), None]):      # lane 4 is region 0: capacity 10
        with pytest.raises(capi.NeedleError) as e:
            m.feed(feed)
        assert e.value.code == INVALID
        assert ([m.lane(k) for k in range(6)], m.stats(), m.ready()) == state
    m.feed([rand_hashes(rng, 7), rand_hashes(rng, 1), None, None, None, None])             # to the brim of both
    assert [m.lane(k)[0] for k in range(6)] == [10, 4, 3, 3, 3, 3]
    for call in (lambda: m.finish([6]), lambda: m.lane(6), lambda: m.feed_from_feeder(capi.Feeder(3))):
        with pytest.raises(capi.NeedleError) as e:
            call()
        assert e.value.code == INVALID
    m.finish([1])
    m.finish([2])
    with pytest.raises(capi.NeedleError) as e:                                   # items for a finished lane, with a good lane beside it
        m.feed([None, None, rand_hashes(rng, 1), None, rand_hashes(rng, 1), None])
    assert e.value.code == INVALID
    assert [m.lane(k) for k in range(6)] == [(10, False), (4, True), (3, True), (3, False), (3, False), (3, False)]
