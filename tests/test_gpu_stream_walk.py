"""-m gpu: the one diagonal walk (csrc/stream_walk.h) through both of its users on the same data: capi.Matcher over four
sources, and a cross-matcher with those sources as residents and one arriving video.  Sources of 1 hash (no cells), 2 (one
cell row), 1 025 (with its n - 1 carried diagonals exactly one workgroup) and 1 026 (one more diagonal); one lane of 1 030
hashes fed three ways.  The checker is the oracle's table DP and the one-shot scan, never one streaming object against the
other; runs are compared as sorted tuples (source, src_end, dst_end, len, src_match_hash, dst_match_hash)."""
import functools

import numpy as np
import pytest

from needle_amd import capi
from tests.test_gpu_crossmatcher import dp, pair_index, rand_hashes
from tests.test_gpu_scan_threshold import _gpu_runs

pytestmark = pytest.mark.gpu

LENS = (1, 2, 1025, 1026)
ITEMS = 1030
SLAB = 4096                                                                      # runs the slab holds at first
STRIP = 512                                                                      # kMaxStrip: a feed is cut into pieces of it
FEEDS = ([1, 511, 512, 6],                                                       # a feed without a cell, then full strips
         [513, 517],                                                             # two pieces each; the second's entering diagonals from item 257 on
         [1030])
CORNER = (2, 1024, 511)                                                          # source, its last row, the last column of a strip in every cutting
# exact copies (source, first row, first column, length)
COPIES = ((2, 300, 1, 12),                                                       # starts at column 1
          (3, 1, 100, 12),                                                       # starts at row 1
          (2, 1005, 492, 20),                                                    # ends in the corner
          (3, 600, 505, 20),                                                     # crosses columns 512 and 513
          (3, 1011, 1015, 15))                                                   # crosses row 1 024, ends in the last row at the last column of all


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


@functools.lru_cache(maxsize=None)
def table():
    rng = np.random.default_rng(41)
    sources = [rand_hashes(rng, n) for n in LENS]
    lane = rand_hashes(rng, ITEMS)
    for s, row, col, length in COPIES:
        sources[s][row: row + length] = lane[col: col + length]           # (copies may share columns, never rows)
    sources[1][1] = lane[511]                                                    # the one cell row's corner, in the same strip column
    for a in sources + [lane]:
        a.setflags(write=False)
    return sources, lane


@functools.lru_cache(maxsize=None)
def expected(t, min_len):
    """Sorted tuples of the final list, from the table DP, checked against the one-shot scan."""
    sources, lane = table()
    want = sorted((s,) + r for s, src in enumerate(sources) for r in dp(src, lane, t, min_len))
    some = [s for s, src in enumerate(sources) if len(src) >= 2]
    shot = _gpu_runs(list(sources) + [lane], [(s, len(sources), min_len) for s in some], t)
    assert sorted((some[k],) + r for k, v in shot.items() for r in v) == want
    return want


def tuples(runs, source_of=None):
    return sorted(((source_of[int(x["problem"])] if source_of else int(x["problem"])), int(x["src_end"]), int(x["dst_end"]), int(x["len"]),
                   int(x["src_match_hash"]), int(x["dst_match_hash"])) for x in runs)


@pytest.mark.parametrize("min_len", (1, 8))
@pytest.mark.parametrize("t", (0, 10))
def test_both_objects_report_the_table_dp_however_the_lane_is_cut(t, min_len):
    sources, lane = table()
    want = expected(t, min_len)
    for s, row, col, length in COPIES:                                           # (the background may lengthen a copy)
        assert any(r[:3] == (s, row + length - 1, col + length - 1) and r[3] >= length for r in want), (s, row, col)
    assert any(r[:3] == CORNER for r in want) and not any(r[0] == 0 for r in want)
    assert any(r[:3] == (1, 1, 511) for r in want) == (min_len == 1)
    last_row = [r for r in want if r[1] == LENS[r[0]] - 1]
    source_of = {pair_index(k, len(sources), len(sources) + 1): k for k in range(len(sources))}
    for feeds in FEEDS:
        assert sum(feeds) == ITEMS
        m = capi.Matcher(sources, [min_len] * len(sources), 1, t)
        x = capi.CrossMatcher.with_resident(sources, 1, [ITEMS], [min_len], t)
        fed = 0
        for n in feeds:
            was = m.stats()[1], x.stats()[1]
            m.feed([lane[fed: fed + n]])
            x.feed([lane[fed: fed + n]])
            fed += n
            rounds = (n + STRIP - 1) // STRIP
            for launches in (m.stats()[1] - was[0], x.stats()[1] - was[1]):
                if len(want) <= SLAB:                                            # three launches per round
                    assert launches == 3 * rounds, (feeds, fed)
                else:                                                            # t = 10, min_len = 1: some 50 000 runs against a slab of 4 096, so this
                    # case doubles as the slab-overflow case of both objects and pins only "a repeated round adds 3"; the other three pin 3 per round
                    assert launches % 3 == 0 and 3 * rounds <= launches <= 6 * rounds, (feeds, fed)
            assert m.ready(0)[1:] == (fed, False) and x.lane(0) == (fed, False)
            # the corner run: the matcher reports it in the round that fed its column, the cross-matcher holds it back
            assert any(r[:3] == CORNER for r in tuples(m.runs(0))) == (fed > CORNER[2]), (feeds, fed)
            assert not any(r[1] == LENS[r[0]] - 1 for r in tuples(x.runs(), source_of)), (feeds, fed)
        # all fed, nothing finished: the closed runs, and for the matcher those in a source's last row
        closed = [r for r in want if r[2] < ITEMS - 1 and r[1] < LENS[r[0]] - 1]
        assert tuples(x.runs(), source_of) == closed, feeds
        assert tuples(m.runs(0)) == sorted(closed + last_row), feeds
        was = m.stats()[1], x.stats()[1]
        m.finish()
        x.finish()
        assert (m.stats()[1] - was[0], x.stats()[1] - was[1]) == (3, 3), feeds
        assert m.ready(0)[2] and x.ready()[1]
        assert tuples(m.runs(0)) == want, feeds
        assert tuples(x.runs(), source_of) == want, feeds
