"""-m gpu: the streaming all-pairs comparator (needle_hip_crossmatcher_*).  The checker is the oracle's table DP, used as
tests/test_gpu_matcher.py uses it (timestamps = row index, min_opening_duration = min_len), and next to it
capi.hamming_runs over the same pairs; runs are compared as sorted lists (src_end, dst_end, len, src_match_hash,
dst_match_hash) per pair, so a run reported twice fails."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from needle_amd import capi, synth
from tests.test_gpu_scan_threshold import _dp_runs, _masks, _popcount

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

THRESHOLDS = (0, 10, 32)
MIN_LENS = (1, 8, 23)
INVALID = capi.ERROR_NAMES.index("InvalidArgument")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def rand_hashes(rng, n):
    return rng.integers(0, 2 ** 32, int(n), dtype=np.uint64).astype(np.uint32)


def pair_index(a, b, n):
    """(a, b), a < b, in the comparator's i-major order."""
    return a * (2 * n - a - 1) // 2 + (b - a - 1)


def pairs_of(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


def by_pair(runs):
    out = {}
    for x in runs:
        out.setdefault(int(x["problem"]), []).append((int(x["src_end"]), int(x["dst_end"]), int(x["len"]),
                                                      int(x["src_match_hash"]), int(x["dst_match_hash"])))
    return {k: sorted(v) for k, v in out.items()}


def nonempty(d):
    return {k: v for k, v in d.items() if v}


def dp(src, dst, t, min_len):
    """The oracle's runs of one pair; a side of fewer than two items has no cell (row 0 and column 0 hold none)."""
    return _dp_runs(src, dst, t, min_len) if len(src) >= 2 and len(dst) >= 2 else []


def oracle(lanes, t, min_len):
    n = len(lanes)
    return nonempty({pair_index(a, b, n): dp(lanes[a], lanes[b], t, min_len) for a, b in pairs_of(n)})


def one_shot(lanes, t, min_len):
    """capi.hamming_runs over the same pairs (those of two lanes that hold anything): {pair: sorted runs}."""
    n = len(lanes)
    some = [(a, b) for a, b in pairs_of(n) if len(lanes[a]) and len(lanes[b])]
    got = by_pair(capi.hamming_runs(list(lanes), [(a, b, min_len) for a, b in some], t))
    return {pair_index(*some[k], n): v for k, v in got.items()}


def stream(lanes, schedule, t, min_len, max_items=None):
    """`schedule`: feeds, each a list with one (first, end) slice or None per lane.  Everything is fed, then finished:
    ({pair: sorted runs}, stats)."""
    n = len(lanes)
    m = capi.CrossMatcher(n, max_items or max(2, max(len(x) for x in lanes)), min_len, t)
    pos = [0] * n
    for feed in schedule:
        chunks = []
        for k, part in enumerate(feed):
            if part is None:
                chunks.append(None)
                continue
            assert part[0] == pos[k] and part[1] <= len(lanes[k])
            chunks.append(lanes[k][part[0]: part[1]])
            pos[k] = part[1]
        m.feed(chunks)
    assert pos == [len(x) for x in lanes] and [m.lane(k) for k in range(n)] == [(len(x), False) for x in lanes]
    assert m.ready()[1] is False
    m.finish()
    assert m.ready()[1] is True and all(m.lane(k)[1] for k in range(n))
    return by_pair(m.runs()), m.stats()


# ---- the planted season -------------------------------------------------------------------------------------------------------
D, A, E, B, C, F = range(6)                     # the lanes, in order
LENS = {D: 2, A: 257, E: 1, B: 300, C: 37, F: 0}


class Planted:
    """Lanes of 2, 257, 1, 300, 37 and 0 hashes on a random background, with structures in several pairs of the first four.
    The table of pair (A, B) -- 257 rows, 300 columns -- is planted as tests/test_gpu_matcher.py plants its table: a
    structure is a stretch of rows a .. a + L - 1 and its own block of columns b .. b + L - 1 with every cell at distance
    exactly t, fenced by a cell at t + 1 at both ends.  C is B's last 37 items: pair (A, C) ends with (A, B)'s run into the
    last column, and pair (B, C) is a run of 36 cells into the corner, the last row and the last column at once.  D's two
    items match A's items 49 and 50 at distance t: a run of one cell in row 1 of pair (D, A), with a matching cell in row 0
    in front of it.  `cuts[lane]`: for every structure its first cell, its last cell and the fence, on the row side (in A)
    and on the column side (in B, and in C where it lies there)."""

    def __init__(self, t, min_len, seed=1):
        rng = np.random.default_rng(seed * 7919 + t * 101 + min_len)
        n, M, T = LENS[A], LENS[B], min(t, 32)
        fence = t + 1 if t + 1 <= 32 else None
        big = rand_hashes(rng, n)
        dst = rand_hashes(rng, M)
        self.t, self.min_len, self.whole = t, min_len, []
        self.cuts = {k: set() for k in LENS}
        L1 = min_len + 1

        def put(a, b, dists, name, before="fence", after="fence"):
            dists = np.asarray(dists, dtype=np.int64)
            L = len(dists)
            assert a >= 1 and a + L <= n and b >= 1 and b + L <= M, (name, a, b, L)
            rows, want = np.arange(a, a + L), dists.copy()
            if before == "match" or (before == "fence" and fence is not None):   # "match": a matching cell in row 0 or column 0
                rows, want = np.concatenate([[a - 1], rows]), np.concatenate([[T if before == "match" else fence], want])
            if after == "fence" and fence is not None and a + L < n and b + L < M:
                rows, want = np.concatenate([rows, [a + L]]), np.concatenate([want, [fence]])
            cols = rows - a + b
            dst[cols] = big[rows] ^ _masks(want, rng, int(rows[0]))
            assert _popcount(big[rows] ^ dst[cols]).tolist() == want.tolist(), name
            self.cuts[A] |= {a, a + 1, a + L - 1, a + L, a + L + 1}
            self.cuts[B] |= {b, b + 1, b + L - 1, b + L, b + L + 1}
            k = 0
            while k < L:                                                         # the stretches at <= t: what the oracle must list
                if dists[k] > t:
                    k += 1
                    continue
                e = k
                while e + 1 < L and dists[e + 1] <= t:
                    e += 1
                if e - k + 1 >= min_len:
                    self.whole.append((name, a + e, b + e, e - k + 1))
                k = e + 1
            return b + L + 2

        # a run from column 1 (column 0 holds a matching cell in front of it) and one from row 1 (row 0 likewise)
        b = put(40, 1, [T] * L1, "starts at j = 1", before="match")
        b = put(1, b + 1, [T] * L1, "starts at i = 1", before="match")
        # exactly min_len, and one cell short of min_len
        b = put(70, b + 1, [T] * min_len, "exactly min_len")
        if min_len > 1:
            b = put(100, b + 1, [T] * (min_len - 1), "min_len - 1")
        # two runs with a single cell at t + 1 between them
        broken = [T] * min_len + [min(t + 1, 32)] + [T] * (min_len + 3)
        self.cuts[A] |= {130 + min_len, 130 + min_len + 1}
        self.cuts[B] |= {b + 1 + min_len, b + 2 + min_len}
        b = put(130, b + 1, broken, "broken by t + 1")
        # a block of equal hashes, 12 rows x 10 columns
        h = np.uint32(rng.integers(0, 2 ** 32))
        big[200:212] = h
        dst[b:b + 10] = h
        self.cuts[A] |= {200, 206, 211, 212}
        self.cuts[B] |= {b, b + 5, b + 9, b + 10}
        b += 12
        b = put(n - L1, b + 1, [T] * L1, "ends at i = n - 1")
        assert b + 1 <= M - L1, (b, min_len)
        put(215, M - L1, [T] * L1, "ends at j = m - 1")
        small = np.array([big[49], big[50]], dtype=np.uint32) ^ _masks([T, T], rng, 0)
        self.cuts[A] |= {49, 50, 51}
        tail = M - LENS[C]
        self.cuts[C] = {c - tail for c in self.cuts[B]}
        self.lanes = [None] * 6
        self.lanes[D], self.lanes[A], self.lanes[E] = small, big, rand_hashes(rng, 1)
        self.lanes[B], self.lanes[C], self.lanes[F] = dst, dst[tail:].copy(), np.zeros(0, dtype=np.uint32)
        for k, n_k in LENS.items():
            assert len(self.lanes[k]) == n_k
            self.cuts[k] = {c for c in self.cuts[k] if 0 < c < n_k}

    _oracle = None

    def oracle(self):
        """{pair: sorted runs} of the whole lanes, computed once."""
        if self._oracle is None:
            self._oracle = oracle(self.lanes, self.t, self.min_len)
            ab, ac, bc, da = (pair_index(*p, 6) for p in ((A, B), (A, C), (B, C), (D, A)))
            if self.t < 32:                                                      # what was planted is there
                for name, i, j, L in self.whole:
                    assert any(r[:3] == (i, j, L) for r in self._oracle[ab]), (name, i, j, L)
                assert (1, 50, 1) in [r[:3] for r in self._oracle.get(da, [])] or self.min_len > 1
            assert len(self._oracle[ab]) >= 6
            assert any(r[1] == LENS[C] - 1 and r[0] < LENS[A] - 1 for r in self._oracle[ac])       # into the last column
            assert any(r[:3] == (LENS[B] - 1, LENS[C] - 1, LENS[C] - 1) for r in self._oracle[bc])  # into the corner
        return self._oracle


_TABLES = {}


def planted(t, min_len):
    if (t, min_len) not in _TABLES:
        _TABLES[(t, min_len)] = Planted(t, min_len)
    return _TABLES[(t, min_len)]


def chunks_from_cuts(cuts, total):
    edges = [0, *sorted(c for c in cuts if 0 < c < total), total]
    return [(a, b) for a, b in zip(edges, edges[1:]) if b > a]


def one_item_per_feed(lens):
    """The lanes alternating: a feed carries one item of one lane."""
    out = []
    for k in range(max(lens)):
        for lane, n in enumerate(lens):
            if k < n:
                out.append([(k, k + 1) if q == lane else None for q in range(len(lens))])
    return out


def whole_lanes(lens, order):
    return [[(0, lens[q]) if q == lane and lens[q] else None for q in range(len(lens))] for lane in order]


def random_schedule(per_lane_chunks, rng):
    """Every lane's chunks in order; which lanes a feed serves is drawn, and some feeds are empty."""
    left = [list(c) for c in per_lane_chunks]
    out = []
    while any(left):
        if rng.random() < 0.05:
            out.append([None] * len(left))
            continue
        out.append([c.pop(0) if c and rng.random() < 0.6 else None for c in left])
    return out


def cuttings(p):
    lens = [len(x) for x in p.lanes]
    n = len(lens)
    yield "one feed", [[(0, x) if x else None for x in lens]]
    yield "one item per feed, the lanes alternating", one_item_per_feed(lens)
    yield "one lane whole before another has anything", whole_lanes(lens, range(n))
    yield "... and the reverse", whole_lanes(lens, reversed(range(n)))
    first = [(0, 1) if x else None for x in lens]
    rest = [(1, x) if x > 1 else None for x in lens]
    yield "a first feed of one item", [first, rest]
    yield "empty feeds", [[None] * n, first, [None] * n, [None] * n, rest, [None] * n]
    for seed in range(5):
        rng = np.random.default_rng(100 + seed)
        per_lane = []
        for k, x in enumerate(lens):
            extra = set(rng.choice(np.arange(1, x), size=int(rng.integers(1, min(20, x))), replace=False).tolist()) if x > 2 else set()
            per_lane.append(chunks_from_cuts(p.cuts[k] | extra, x))
        yield f"random {seed}", random_schedule(per_lane, rng)


# ---- 1. any cutting of both sides equals the one-shot and the oracle ---------------------------------------------------------
@pytest.mark.parametrize("min_len", MIN_LENS)
@pytest.mark.parametrize("t", THRESHOLDS)
def test_any_cutting_of_both_sides_equals_the_one_shot_and_the_oracle(t, min_len):
    p = planted(t, min_len)
    want = p.oracle()
    assert one_shot(p.lanes, t, min_len) == want
    for name, schedule in cuttings(p):
        got, _ = stream(p.lanes, schedule, t, min_len)
        assert got == want, name


# ---- 2. reported when the rule says so ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_len", MIN_LENS)
@pytest.mark.parametrize("t", THRESHOLDS)
def test_runs_are_reported_when_the_rule_says_so(t, min_len):
    """Lane a holds rows [0, Ja), lane b columns [0, Jb): the pair has reported exactly the runs of the prefixes' list with
    src_end < Ja - 1 and dst_end < Jb - 1."""
    p = planted(t, min_len)
    lens = [len(x) for x in p.lanes]
    n = len(lens)
    m = capi.CrossMatcher(n, max(lens), min_len, t)
    fed = [0] * n
    before, closed = [], {}
    for feed in one_item_per_feed(lens):
        lane = next(k for k, part in enumerate(feed) if part is not None)
        m.feed([None if part is None else p.lanes[k][part[0]: part[1]] for k, part in enumerate(feed)])
        fed[lane] += 1
        assert m.lane(lane) == (fed[lane], False)
        raw = m.runs()
        now = [tuple(int(v) for v in x) for x in raw]
        assert now[:len(before)] == before, fed                                  # appended, never revised
        before = now
        for a, b in pairs_of(n):                                                 # (only this lane's pairs have changed)
            if lane in (a, b):
                runs = dp(p.lanes[a][:fed[a]], p.lanes[b][:fed[b]], t, min_len)
                closed[pair_index(a, b, n)] = [r for r in runs if r[0] < fed[a] - 1 and r[1] < fed[b] - 1]
        assert by_pair(raw) == nonempty(closed), fed
    assert m.ready() == (len(before), False)
    m.finish()
    assert by_pair(m.runs()) == p.oracle()
    assert [tuple(int(v) for v in x) for x in m.runs()][:len(before)] == before


# ---- 3. lanes out of step -----------------------------------------------------------------------------------------------------
def test_lanes_out_of_step():
    rng = np.random.default_rng(5)
    t, min_len = 10, 4
    lengths = (2, 57, 400, 129, 256)
    lanes = [rand_hashes(rng, x) for x in lengths]
    # copies of stretches of an earlier lane with a few bits flipped; (1, 3) holds a run into lane 1's last row, which is
    # open until lane 3 finishes too
    for a, b, ra, cb, L in ((1, 2, 10, 300, 30), (1, 3, 57 - 20, 60, 20), (2, 3, 350, 100, 25), (2, 4, 1, 200, 45),
                            (3, 4, 100, 256 - 12, 12), (1, 4, 5, 5, 40)):
        lanes[b][cb: cb + L] = lanes[a][ra: ra + L] ^ _masks([3] * L, rng, 0)
    n = len(lanes)
    want = oracle(lanes, t, min_len)
    assert one_shot(lanes, t, min_len) == want
    assert all(pair_index(a, b, n) in want for a, b in ((1, 2), (1, 3), (2, 3), (2, 4), (3, 4), (1, 4)))
    p13 = pair_index(1, 3, n)
    assert any(r[0] == lengths[1] - 1 for r in want[p13])

    def rule(m):
        """Every pair that is not complete has reported what the rule says, a complete one everything."""
        fed = [m.lane(k) for k in range(n)]
        exp = {}
        for a, b in pairs_of(n):
            runs = dp(lanes[a][:fed[a][0]], lanes[b][:fed[b][0]], t, min_len)
            if not (fed[a][1] and fed[b][1]):
                runs = [r for r in runs if r[0] < fed[a][0] - 1 and r[1] < fed[b][0] - 1]
            exp[pair_index(a, b, n)] = runs
        assert by_pair(m.runs()) == nonempty(exp), fed

    m = capi.CrossMatcher(n, 400, min_len, t)
    pos = [0] * n
    step = 0
    while any(pos[k] < lengths[k] for k in range(n)):
        chunk = []
        for k in range(n):
            take = 0 if (step + k) % 3 == 0 else int(rng.integers(0, 70))        # some lanes get nothing
            chunk.append(lanes[k][pos[k]: pos[k] + take] if take else None)
            pos[k] = min(lengths[k], pos[k] + take)
        m.feed(chunk)
        step += 1
        if pos[1] == lengths[1] and not m.lane(1)[1]:                            # lane 1 finishes early, the others go on
            m.finish([1])
            assert m.lane(1) == (lengths[1], True) and not m.ready()[1]
            rule(m)                                                              # its open runs wait for the other lanes
        if pos[3] == lengths[3] and m.lane(1)[1] and not m.lane(3)[1]:           # two finished lanes: their pair is complete at once
            m.finish([3])
            assert by_pair(m.runs()).get(p13) == want[p13]
            rule(m)
        if m.lane(1)[1] and step % 2:
            state = ([m.lane(k) for k in range(n)], m.stats(), m.ready())
            with pytest.raises(capi.NeedleError) as e:                           # refused as a whole: no lane moves
                m.feed([lanes[0][:0], lanes[1][:5], lanes[2][:1] if pos[2] < lengths[2] else None, None, None])
            assert e.value.code == INVALID
            assert ([m.lane(k) for k in range(n)], m.stats(), m.ready()) == state
        if step % 4 == 0:
            rule(m)
    assert m.lane(1)[1] and m.lane(3)[1] and [m.lane(k)[0] for k in range(n)] == list(lengths)
    m.finish()
    assert m.ready()[1] and by_pair(m.runs()) == want
    m.finish()                                                                   # nothing left: nothing happens
    assert by_pair(m.runs()) == want
    # the errors that need an object
    some = rand_hashes(rng, 3)
    fresh = capi.CrossMatcher(n, 10, min_len, t)
    for call in (lambda: m.finish([5]), lambda: m.lane(5), lambda: m.runs(0, m.ready()[0] + 1), lambda: m.runs(m.ready()[0] + 1, 0),
                 lambda: m.feed([None, None, some, None, None]),                 # items for a finished lane
                 lambda: m.feed_from_feeder(capi.Feeder(4)),                     # unequal lane counts
                 lambda: fresh.feed([None, rand_hashes(rng, 11), None, None, None]),   # past max_items in one feed
                 lambda: fresh.finish([0, 7])):
        with pytest.raises(capi.NeedleError) as e:
            call()
        assert e.value.code == INVALID
    fresh.feed([None, rand_hashes(rng, 6), None, None, None])
    with pytest.raises(capi.NeedleError) as e:                                   # ... and over two
        fresh.feed([some, rand_hashes(rng, 5), None, None, None])
    assert e.value.code == INVALID and [fresh.lane(k)[0] for k in range(n)] == [0, 6, 0, 0, 0]
    fresh.feed([some, rand_hashes(rng, 4), None, None, None])
    assert [fresh.lane(k) for k in range(n)] == [(3, False), (10, False), (0, False), (0, False), (0, False)]


# ---- 4. every cell once, fixed launches ---------------------------------------------------------------------------------------
def test_every_cell_once_and_fixed_launches():
    p = planted(10, 8)
    lens = [len(x) for x in p.lanes]
    schedule = one_item_per_feed(lens)
    _, (feeds, launches, cells, _) = stream(p.lanes, schedule, 10, 8)
    assert feeds == len(schedule) == sum(lens)
    assert cells == sum(max(lens[a] - 1, 0) * max(lens[b] - 1, 0) for a, b in pairs_of(len(lens)))
    per_round = launches // (feeds + 1)                                          # the finish is a round as well
    assert per_round >= 1 and launches == per_round * (feeds + 1)

    rng = np.random.default_rng(8)
    for n in (3, 12):                                                            # the same count for 3 lanes and for 12
        m = capi.CrossMatcher(n, 200, 3, 10)
        chunk = rand_hashes(rng, 6)
        state = []
        for k in range(30):
            was = m.stats()[1]
            m.feed([chunk if (k + lane) % 2 else None for lane in range(n)])     # only the lanes with data differ
            assert m.stats()[1] - was == per_round, (n, k)
            state.append(m.stats()[3])
        was = m.stats()[1]
        m.feed([chunk] + [None] * (n - 1))                                       # one lane alone
        assert m.stats()[1] - was == per_round
        m.finish([0])
        m.finish()
        assert m.stats()[1] - was == 3 * per_round and m.stats()[0] == 31
        assert len(set(state)) == 1 and state[0] >= capi.CrossMatcher.state_bytes(n, 200)


# ---- 5. slab overflow ---------------------------------------------------------------------------------------------------------
_SLAB_CHILD = """
import json, sys
import numpy as np
from needle_amd import capi
from tests.test_gpu_crossmatcher import by_pair
lanes = [np.full(64, 0x5A5A5A5A, dtype=np.uint32) for _ in range(3)]
m = capi.CrossMatcher(3, 64, 8, 10)
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


def test_a_slab_too_small_loses_nothing():
    src = np.full(64, 0x5A5A5A5A, dtype=np.uint32)
    want = _dp_runs(src, src, 10, 8)
    assert len(want) > 100                                                       # every diagonal of 8 cells or more is a run
    small, roomy = _slab_child(4), _slab_child(0)
    for child in (small, roomy):
        assert sorted(child["runs"]) == ["0", "1", "2"]
        for runs in child["runs"].values():
            assert [tuple(r) for r in runs] == want
    assert small["stats"][1] > roomy["stats"][1]                                 # the repeated rounds
    assert small["stats"][0] == roomy["stats"][0] == 4
    assert "NEEDLE_HIP_CROSSMATCHER_RUN_SLAB" not in os.environ


# ---- 6. the paths the small tables do not take --------------------------------------------------------------------------------
def test_feeds_wider_than_a_piece_on_both_sides():
    """Lanes of 700 / 1300 / 600 items in single feeds: both lanes of a pair are cut into 512-item pieces in the same feed.
    Runs cross the (512, 512) and (512, 1024) corners of pair (0, 1), one ends in the last row of a piece and one starts in
    the first row of the next, and the other pairs hold runs across their own piece boundaries."""
    rng = np.random.default_rng(21)
    lanes = [rand_hashes(rng, x) for x in (700, 1300, 600)]
    copies = ((0, 1, 480, 480, 80), (0, 1, 500, 1012, 40), (0, 1, 512 - 30, 600, 30), (0, 1, 512, 640, 30), (0, 1, 640, 1, 59),
              (0, 1, 2, 1240, 60), (0, 2, 490, 490, 50), (1, 2, 1000, 440, 40), (1, 2, 1250, 550, 50))
    for a, b, ra, cb, L in copies:
        lanes[b][cb: cb + L] = lanes[a][ra: ra + L] ^ _masks([2] * L, rng, 0)
    t, min_len = 9, 12
    want = oracle(lanes, t, min_len)
    for a, b, ra, cb, L in copies:                                               # (the background may lengthen a copy)
        assert any(r[:2] == (ra + L - 1, cb + L - 1) and r[2] >= L for r in want[pair_index(a, b, 3)]), (a, b, ra, cb)
    assert one_shot(lanes, t, min_len) == want
    whole = [(0, len(x)) for x in lanes]
    got, stats = stream(lanes, [whole], t, min_len)
    assert got == want
    per_round = stats[1] // 4                                                    # pieces of 512: three rounds, and the finish
    assert stats[0] == 1 and stats[1] == 4 * per_round
    assert stats[2] == sum((len(lanes[a]) - 1) * (len(lanes[b]) - 1) for a, b in pairs_of(3))
    for schedule in ([[(0, 700), None, None], [None, (0, 1300), (0, 600)]],
                     [[None, (0, 3), (0, 600)], [(0, 600), (3, 1300), None], [(600, 700), None, None]]):
        got, _ = stream(lanes, schedule, t, min_len)
        assert got == want, schedule


def test_a_lane_of_65540_items_takes_the_32_bit_state():
    rng = np.random.default_rng(22)
    long_lane = rand_hashes(rng, 65540)
    before, after = rand_hashes(rng, 48), rand_hashes(rng, 48)
    long_lane[65520:65540] = before[10:30] ^ _masks([1] * 20, rng, 0)            # a run into column 65 539 of pair (0, 1)
    after[5:45] = long_lane[65500:65540] ^ _masks([1] * 40, rng, 0)              # ... and one into row 65 539 of pair (1, 2)
    lanes = [before, long_lane, after]
    want = oracle(lanes, 9, 5)
    assert any(r[:2] == (65539, 44) and r[2] >= 40 for r in want[pair_index(1, 2, 3)])
    assert any(r[:2] == (29, 65539) and r[2] >= 20 for r in want[pair_index(0, 1, 3)])
    assert one_shot(lanes, 9, 5) == want
    assert capi.CrossMatcher.state_bytes(3, 65540) == 3 * 4 * 65540 * 4 + 3 * 65540 * 4
    got, stats = stream(lanes, [[(0, 20), (0, 30000), None], [(20, 21), (30000, 65540), (0, 48)], [(21, 48), None, None]], 9, 5, max_items=65540)
    assert got == want
    assert stats[2] == sum((len(lanes[a]) - 1) * (len(lanes[b]) - 1) for a, b in pairs_of(3))


# ---- 7. from a feeder, to results ---------------------------------------------------------------------------------------------
def _results(res):
    return [None if r is None else (r.opening, r.ending) for r in res]


def _from_a_feeder_to_results():
    seconds = (60.0, 75.0, 90.0, 70.0)
    pcms = [synth.make_episode(k, s, 20.0).pcm for k, s in enumerate(seconds)]   # every episode holds the same 20 s intro
    n, t, min_len = len(pcms), 10, 30
    items = capi.fingerprint(pcms, 1, 2)
    want = one_shot(items, t, min_len)
    assert sorted(want) == list(range(6)) and min(max(r[2] for r in runs) for runs in want.values()) >= 60   # 20 s: ~80 kept items
    f = capi.Feeder(n, 1, 11025, capi.SAMPLE_S16, 2)
    m = capi.CrossMatcher(n, max(len(x) for x in items), min_len, t)
    half = 11025 // 2
    pos = [0] * n
    step, early = 0, 0
    while not m.ready()[1]:
        chunk = []
        for k in range(n):
            take = 0 if (step + k) % 3 == 0 else half                            # the lanes out of step
            chunk.append(pcms[k][pos[k]: pos[k] + take] if take and pos[k] < len(pcms[k]) else None)
            pos[k] = min(len(pcms[k]), pos[k] + take)
        f.feed(chunk)
        ended = [k for k in range(n) if pos[k] == len(pcms[k]) and not f.ready(k)[2]]
        if ended:
            f.finish(ended)
        if not all(f.ready(k)[2] for k in range(n)):
            m.feed_from_feeder(f)
            assert [m.lane(k) for k in range(n)] == [(f.ready(k)[0], f.ready(k)[2]) for k in range(n)]
            early = max(early, max((int(x["len"]) for x in m.runs()), default=0))
            assert not m.ready()[1]
        else:
            assert early >= 60, "a shared segment's run is reported before the last lane finishes"
            m.feed_from_feeder(f)
        step += 1
    assert [m.lane(k) for k in range(n)] == [(len(x), True) for x in items]
    runs = m.runs()
    assert by_pair(runs) == want
    m.feed_from_feeder(f)                                                        # nothing new: nothing happens
    assert by_pair(m.runs()) == want
    fhs = [f.frame_hashes(k) for k in range(n)]
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(n)], min_opening_duration=10)
    got, ref = _results(cmp.results_from_runs(fhs, runs)), _results(cmp.run_with_frame_hashes(fhs))
    assert got == ref
    assert all(r is not None and r[0] is not None for r in ref)


def test_from_a_feeder_to_results():
    _from_a_feeder_to_results()


def test_from_a_feeder_to_results_f64(monkeypatch):
    monkeypatch.setenv("NEEDLE_HIP_STFT", "f64")
    _from_a_feeder_to_results()


# ---- 8. existing paths untouched ----------------------------------------------------------------------------------------------
def test_existing_paths_launch_no_crossmatcher_kernel():
    eps = synth.make_library(3, 60.0, 15.0)
    pcms = [e.pcm for e in eps]
    p = planted(10, 8)
    names = ("crossmatch_land", "crossmatch_walk", "crossmatch_simhash")
    capi.set_kernel_timing("all,sum")
    try:
        one_shot(p.lanes, 10, 8)
        lib = capi.Library(len(pcms))
        lib.set_pcm(pcms, [len(x) for x in pcms])
        cmp = capi.Comparator([f"ep{k}.wav" for k in range(len(pcms))], min_opening_duration=10)
        lib.job_begin(cmp, 0)
        lib.job_end(cmp, 0)
        mt = capi.Matcher([p.lanes[A]], [8], 1, 10)
        mt.feed([p.lanes[B]])
        mt.finish()
        capi.synchronize()
        assert capi.last_kernel_ms("simhash_runs") >= 0 or capi.last_kernel_ms("hamming_runs") >= 0
        assert capi.last_kernel_ms("matcher_strip") >= 0
        assert all(capi.last_kernel_ms(k) < 0 for k in names), "no crossmatcher kernel in a one-shot scan, a library job or a Matcher feed"
        stream(p.lanes, [[(0, len(x)) if len(x) else None for x in p.lanes]], 10, 8)
        capi.synchronize()
        assert all(capi.last_kernel_ms(k) >= 0 for k in names)
    finally:
        capi.set_kernel_timing(None)
