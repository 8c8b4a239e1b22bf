"""-m gpu: regions in the streaming comparator (needle_hip_matcher_new_regions; csrc/matcher.hip).  Source s is in region
s % 2 and lane l in region l % 2, and a lane meets its own region's sources only.  The reference of every lane is
needle_hip_hamming_runs_host over the (source, lane) problems of the lane's region; runs are compared as sorted tuples
(src_end, dst_end, len, src_match_hash, dst_match_hash) per source.  What can go wrong is the region of a workgroup (the
workgroup list is ordered by region and the two regions own different numbers of workgroups), the place of a lane's state
(a lane holds its own region's frontiers only), and a source without cells, which keeps its index."""
import numpy as np
import pytest

from needle_amd import capi
from tests.test_gpu_matcher import by_source, nonempty
from tests.test_gpu_scan_threshold import _masks

pytestmark = pytest.mark.gpu
T = 10
# region 0: 1030 (crosses the 1024-row block of carried diagonals), 300, 2; region 1: 37, 0 (no cells), 257
SOURCE_LENS = (1030, 37, 300, 0, 2, 257)
MIN_LENS = (6, 5, 4, 3, 1, 7)
LANE_LENS = (700, 650, 601, 620)                                                 # two videos x two regions
# (source, first row, lane, first column, length): copies with a few bits flipped.  Same region ...
PLANTED = ((0, 1000, 0, 40, 30),                                                 # into the last row of 1030, across row 1024
           (0, 5, 2, 500, 90), (2, 100, 0, 505, 40),                             # across column 512
           (2, 260, 2, 1, 40),                                                   # into the last row of 300, from column 1
           (4, 0, 0, 300, 2),                                                    # the source of two rows: one cell
           (1, 7, 1, 600, 30),                                                   # into the last row of 37, to column 629
           (5, 1, 3, 580, 40), (5, 200, 1, 10, 57), (1, 0, 3, 0, 20))
# ... and, as bait, across regions: a lane must not meet these sources
BAIT = ((0, 200, 1, 100, 50), (2, 20, 3, 200, 60), (5, 50, 0, 100, 50), (1, 2, 2, 300, 30), (0, 600, 3, 400, 80))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


class Table:
    def __init__(self, seed=3):
        rng = np.random.default_rng(seed)
        new = lambda n: rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        self.sources = [new(n) for n in SOURCE_LENS]
        self.lanes = [new(n) for n in LANE_LENS]
        self.again = new(333)                                                    # what lane 1 is reused for
        for s, a, l, b, L in PLANTED + BAIT:
            self.lanes[l][b:b + L] = self.sources[s][a:a + L] ^ _masks([3] * L, rng, 0)
        self.again[50:80] = self.sources[1][7:37] ^ _masks([2] * 30, rng, 0)
        self.again[100:150] = self.sources[0][300:350]                           # bait
        self._want = {}

    def reference(self, lane, dst, min_lens=MIN_LENS):
        """{source: sorted runs}: the one-shot scan over the lane's own region's sources (those long enough to hold a cell)."""
        mine = [s for s in range(len(SOURCE_LENS)) if s % 2 == lane % 2 and SOURCE_LENS[s] >= 2 and min_lens[s]]
        runs = capi.hamming_runs([*[self.sources[s] for s in mine], dst], [(q, len(mine), min_lens[s]) for q, s in enumerate(mine)], T)
        return {mine[q]: v for q, v in by_source(runs).items()}

    def want(self, lane):
        if lane not in self._want:
            self._want[lane] = self.reference(lane, self.lanes[lane])
        return self._want[lane]


_TABLE = []


@pytest.fixture(scope="module")
def table():
    if not _TABLE:
        t = Table()
        for s, a, l, b, L in PLANTED:                                            # what was planted is there
            assert s % 2 == l % 2
            if L >= MIN_LENS[s]:
                assert any(r[0] >= a + L - 1 and r[0] - r[1] == a - b and r[2] >= L - 1 for r in t.want(l)[s]), (s, a, l, b, L)
        assert all(s % 2 != l % 2 for s, _, l, _, _ in BAIT)
        assert {s for l in range(4) for s in t.want(l)} == {0, 1, 2, 4, 5}, "every source that has cells"
        _TABLE.append(t)
    return _TABLE[0]


def _strips(n):
    return -(-n // 512)


def stream(table, feeds, make=None):
    """Every lane fed by `feeds` (a list of per-lane sizes), then all finished at once: (matcher, rounds)."""
    m = make() if make else capi.Matcher.with_regions(table.sources, MIN_LENS, 2, 4, T)
    pos, rounds = [0] * 4, 0
    for sizes in feeds:
        chunk = [table.lanes[l][pos[l]: pos[l] + sizes[l]] if sizes[l] else None for l in range(4)]
        taken = [0 if c is None else len(c) for c in chunk]
        m.feed(chunk)
        pos = [p + k for p, k in zip(pos, taken)]
        rounds += _strips(max(taken))
    assert pos == list(LANE_LENS) and [m.ready(l)[1:] for l in range(4)] == [(n, False) for n in LANE_LENS]
    m.finish()
    assert [m.ready(l)[1:] for l in range(4)] == [(n, True) for n in LANE_LENS]
    return m, rounds + 1


def cuttings():
    yield "one feed", [LANE_LENS]
    yield "one item per feed", [tuple(1 if k < n else 0 for n in LANE_LENS) for k in range(max(LANE_LENS))]
    rng = np.random.default_rng(17)
    ragged, left = [], list(LANE_LENS)
    while any(left):
        sizes = tuple(0 if rng.random() < 0.3 else min(left[l], int(rng.integers(1, 160))) for l in range(4))
        left = [a - b for a, b in zip(left, sizes)]
        ragged.append(sizes)
        if rng.random() < 0.1:
            ragged.append((0, 0, 0, 0))
    assert any(0 in s and any(s) for s in ragged) and (0, 0, 0, 0) in ragged
    yield "ragged feeds with empty ones", ragged
    yield "one feed of 600 items", [(600,) * 4, tuple(n - 600 for n in LANE_LENS)]


def state_bytes(min_lens=MIN_LENS, lanes=4):
    """The per-region arithmetic of stats[3] less the histories: the sources, and two sets of 2-byte run lengths per lane
    over the hashes of its own region's sources that have cells."""
    rows = [sum(n for s, n in enumerate(SOURCE_LENS) if s % 2 == r and n >= 2 and min_lens[s]) for r in range(2)]
    return 4 * sum(SOURCE_LENS) + 2 * 2 * sum(rows[l % 2] for l in range(lanes))


# ---- 1. every cutting equals the one-shot scan of the lane's own region ----------------------------------------------------------
@pytest.mark.parametrize("name,feeds", list(cuttings()), ids=[n for n, _ in cuttings()])
def test_every_cutting_equals_the_one_shot_of_its_own_region(table, name, feeds):
    m, rounds = stream(table, feeds)
    for lane in range(4):
        got = by_source(m.runs(lane))
        assert got == nonempty(table.want(lane)), (name, lane)
        assert all(s % 2 == lane % 2 for s in got), "no run has a source of the other region"
    feeds_with_items = sum(1 for s in feeds if any(s))
    stats = m.stats()
    assert stats[0] == feeds_with_items and stats[1] == 3 * rounds, name
    assert stats[3] == state_bytes() + 4 * sum(LANE_LENS)


def test_the_two_regions_own_different_numbers_of_workgroups():
    """What the table above stands on: 1030 rows need two blocks of carried diagonals, every other source one."""
    blocks = [sum(-(-(n - 1) // 1024) for s, n in enumerate(SOURCE_LENS) if s % 2 == r and n >= 2) for r in range(2)]
    assert blocks == [4, 2]


# ---- 2. a source that can hold no run ---------------------------------------------------------------------------------------------
def test_a_source_with_min_len_zero_keeps_its_index_and_has_no_state(table):
    mins = (6, 5, 0, 3, 1, 7)                                                    # the source of 300: no cells, no workgroups, no state
    m, rounds = stream(table, [LANE_LENS], make=lambda: capi.Matcher.with_regions(table.sources, mins, 2, 4, T))
    for lane in range(4):
        want = nonempty(table.reference(lane, table.lanes[lane], mins))
        assert by_source(m.runs(lane)) == want and 2 not in want, lane
    assert 0 in by_source(m.runs(0)) and 0 in by_source(m.runs(2)) and 2 in table.want(0) and 2 in table.want(2)
    assert m.stats()[1] == 3 * rounds
    assert m.stats()[3] == state_bytes(mins) + 4 * sum(LANE_LENS) == state_bytes() - 2 * 2 * 2 * 300 + 4 * sum(LANE_LENS)
    with pytest.raises(capi.NeedleError) as e:                                   # the old constructor keeps refusing it
        capi.Matcher(table.sources, mins, 4, T)
    assert e.value.code == capi.ERROR_NAMES.index("InvalidArgument") and "min_len" in str(e.value)
    # a region none of whose sources has a cell: its lanes only count
    only = capi.Matcher.with_regions(table.sources, (6, 0, 4, 3, 1, 0), 2, 4, T)
    only.feed([x[:100] for x in table.lanes])
    only.feed([x[100:] for x in table.lanes])
    assert len(only.open(1)) == 0
    only.finish()
    assert [only.ready(l)[1:] for l in range(4)] == [(n, True) for n in LANE_LENS]
    assert len(only.runs(1)) == 0 and len(only.runs(3)) == 0
    assert by_source(only.runs(0)) == nonempty(table.want(0)) and by_source(only.runs(2)) == nonempty(table.want(2))


# ---- 3. one region through the new constructor is the old matcher ---------------------------------------------------------------
def test_one_region_is_the_old_matcher_run_for_run(table):
    sources = [s for s in table.sources if len(s)]
    mins = [m for m, s in zip(MIN_LENS, table.sources) if len(s)]
    old, new = capi.Matcher(sources, mins, 2, T), capi.Matcher.with_regions(sources, mins, 1, 2, T)
    for a, b in ((0, 1), (1, 300), (300, 601)):
        for m in (old, new):
            m.feed([table.lanes[0][a:b], table.lanes[1][a:b] if a else None])
        for lane in range(2):                                                    # the same runs after every feed, not only at the end
            assert sorted(map(tuple, old.runs(lane).tolist())) == sorted(map(tuple, new.runs(lane).tolist())), (b, lane)
            assert sorted(map(tuple, old.open(lane).tolist())) == sorted(map(tuple, new.open(lane).tolist())), (b, lane)
    for m in (old, new):
        m.finish()
    for lane in range(2):
        runs = sorted(map(tuple, old.runs(lane).tolist()))
        assert runs == sorted(map(tuple, new.runs(lane).tolist())) and (len(runs) >= 3 or lane), lane
    assert {int(x) for x in old.runs(0)["problem"]} >= {0, 2, 4}, "with one region lane 0 meets what is bait with two (source 5, here 4)"
    assert old.stats() == new.stats()


# ---- 4. reset of one lane, and open ---------------------------------------------------------------------------------------------
def test_reset_of_one_lane_and_open(table):
    m = capi.Matcher.with_regions(table.sources, MIN_LENS, 2, 4, T)
    J = 620                                                                      # lane 1 holds a run open at column 619
    m.feed([x[:J] for x in table.lanes])
    counts = [m.ready(l)[0] for l in range(4)]
    for lane in range(4):
        prefix = table.reference(lane, table.lanes[lane][:J])
        n = lambda s: SOURCE_LENS[s]
        still = {s: [(r[0], r[1], r[2], 0, 0) for r in runs if r[1] == J - 1 and r[0] < n(s) - 1] for s, runs in prefix.items()}
        closed = {s: [r for r in runs if r[1] < J - 1 or (r[0] == n(s) - 1 and r[1] <= J - 1)] for s, runs in prefix.items()}
        opened = m.open(lane)
        assert by_source(opened) == nonempty(still), lane
        assert by_source(m.runs(lane)) == nonempty(closed), lane
        assert by_source(m.open(lane)) == by_source(opened) and m.ready(lane)[0] == counts[lane]   # a function of the state alone
    assert by_source(m.open(1)), "a run is open on lane 1"
    m.feed([x[J:] for x in table.lanes])
    m.finish([1])
    assert by_source(m.runs(1)) == nonempty(table.want(1)) and m.ready(1)[1:] == (LANE_LENS[1], True)
    with pytest.raises(capi.NeedleError) as e:                                   # refused as a whole: a finished lane before reset
        m.feed([None, table.again[:5], None, None])
    assert e.value.code == capi.ERROR_NAMES.index("InvalidArgument")
    m.reset([1])
    assert m.ready(1) == (0, 0, False) and len(m.open(1)) == 0
    for a in range(0, len(table.again), 41):
        m.feed([None, table.again[a:a + 41], None, None])
    m.finish()
    want = nonempty(table.reference(1, table.again))
    assert by_source(m.runs(1)) == want and set(want) == {1}, "the reused lane meets its own region only"
    for lane in (0, 2, 3):                                                       # the other lanes went on as if nothing happened
        assert by_source(m.runs(lane)) == nonempty(table.want(lane)), lane
    assert len(m.open(0)) == 0
    invalid = capi.ERROR_NAMES.index("InvalidArgument")
    for call in (lambda: m.finish([4]), lambda: m.reset([4]), lambda: m.ready(4), lambda: m.runs(4), lambda: m.open(4),
                 lambda: m.feed_from_feeder(capi.Feeder(3))):
        with pytest.raises(capi.NeedleError) as e:
            call()
        assert e.value.code == invalid
