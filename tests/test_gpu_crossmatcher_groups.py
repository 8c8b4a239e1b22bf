"""-m gpu: groups of videos in the streaming all-pairs comparator (needle_hip_crossmatcher_new_grouped; the live-pair table:
needle_amd/csrc/cross_pairs.h; the walk's listed policy: needle_amd/csrc/crossmatch.hip).  The checker is the oracle's table DP
per same-label pair with an arriving end, numbered by the NumPy model of the grouped ids (tests/group_ids.py); runs are compared
as sorted lists (src_end, dst_end, len, src_match_hash, dst_match_hash) per problem, so a lost run, a doubled run, a run under
the wrong problem and any run of a cross-label or resident-resident pair fails."""
import numpy as np
import pytest

from needle_amd import capi
from tests import best_match_model as M
from tests import group_ids as G
from tests.test_gpu_crossmatcher import (LENS, by_pair, chunks_from_cuts, dp, nonempty, one_item_per_feed, pair_index, pairs_of, planted,
                                         rand_hashes, random_schedule, whole_lanes)
from tests.test_gpu_feeder_formats import timed
from tests.test_gpu_grouped import Videos, _as, even_timestamps, random_rows
from tests.test_gpu_scan_threshold import _masks

pytestmark = pytest.mark.gpu
SLAB = 32 + 4096 * 24                                                            # the run slab's first size
INVALID = capi.ERROR_NAMES.index("InvalidArgument")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def oracle_live(rows, labels, k, t, min_len, regions=1):
    """{problem: sorted runs} of the table DP over the live problems; rows[video * regions + region] over all videos."""
    return nonempty({pid * regions + r: dp(rows[a * regions + r], rows[b * regions + r], t, min_len[r])
                     for (a, b), pid in G.live_pairs(labels, k).items() for r in range(regions)})


def live_cells(rows, labels, k, regions=1):
    return sum(max(len(rows[a * regions + r]) - 1, 0) * max(len(rows[b * regions + r]) - 1, 0)
               for a, b in G.live_pairs(labels, k) for r in range(regions))


def new(rows, labels, k, max_items, min_len, t):
    regions = len(max_items)
    m = capi.CrossMatcher.with_groups(labels[k:], max_items, min_len, t, resident=rows[:k * regions], resident_groups=labels[:k])
    videos = len(labels) - k
    assert m.resident == k and m.shape() == (videos, regions) and m.lanes == videos * regions
    assert m.groups.tolist() == list(labels)
    return m


def feed(m, lanes, schedule):
    """`schedule`: feeds, each a list with one (first, end) slice or None per lane; ("finish", lanes) steps between them."""
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


def stream(rows, labels, k, schedule, t, max_items, min_len):
    """Everything is fed, then what is left is finished: ({problem: sorted runs}, stats)."""
    regions = len(max_items)
    m = new(rows, labels, k, max_items, min_len, t)
    feed(m, rows[k * regions:], schedule)
    m.finish()
    assert m.ready()[1] is True
    return by_pair(m.runs()), m.stats()


def one_feed(lanes):
    return [[(0, len(x)) if len(x) else None for x in lanes]]


# ---- 1. two copies of the planted season under two labels ------------------------------------------------------------------------
TWO_SEASONS = [1, 2] * 6 + [3]                                                   # video 2 i + c: lane i of copy c; one lane alone


def two_seasons(p):
    alone = rand_hashes(np.random.default_rng(77), 50)
    alone[5:45] = p.lanes[1][100:140]                                            # ... which shares 40 hashes with both copies' A
    return [p.lanes[i] for i in range(6) for _ in range(2)] + [alone]


def two_season_cuttings(p, lanes):
    lens = [len(x) for x in lanes]
    yield "one item per feed, the lanes alternating", one_item_per_feed(lens)
    yield "one lane whole before another has anything", whole_lanes(lens, range(len(lens)))
    yield "... and the reverse", whole_lanes(lens, reversed(range(len(lens))))
    for seed in range(2):
        rng = np.random.default_rng(200 + seed)
        per_lane = []
        for v, x in enumerate(lens):
            cuts = p.cuts[v // 2] if v < 12 else set()
            extra = set(rng.choice(np.arange(1, x), size=int(rng.integers(1, min(20, x))), replace=False).tolist()) if x > 2 else set()
            per_lane.append(chunks_from_cuts(cuts | extra, x))                   # (the two copies are cut differently)
        yield f"random {seed}", random_schedule(per_lane, rng)


@pytest.mark.parametrize("min_len", (1, 23))
@pytest.mark.parametrize("t", (0, 10))
def test_two_copies_of_the_planted_season_under_two_labels(t, min_len):
    """Both copies hold the same hashes, so every cross-label pair has the runs of its same-label twin: an ungrouped matcher
    reports them all."""
    p = planted(t, min_len)
    lanes = two_seasons(p)
    ids = G.live_pairs(TWO_SEASONS, 0)
    assert len(ids) == 30 and all(TWO_SEASONS[a] == TWO_SEASONS[b] for a, b in ids)
    want = {ids[(2 * a + c, 2 * b + c)]: runs for c in range(2) for (a, b) in pairs_of(6)
            for runs in [p.oracle().get(pair_index(a, b, 6))] if runs}
    assert want == oracle_live(lanes, TWO_SEASONS, 0, t, [min_len]) and len(want) >= 6   # (A, B), (A, C), (B, C) of both copies
    # two ungrouped cross-matchers, re-numbered
    renumbered = {}
    for c in range(2):
        plain = capi.CrossMatcher(6, 300, min_len, t)
        plain.feed([x if len(x) else None for x in lanes[c:12:2]])
        plain.finish()
        for prob, runs in by_pair(plain.runs()).items():
            a, b = pairs_of(6)[prob]
            renumbered[ids[(2 * a + c, 2 * b + c)]] = runs
    assert renumbered == want
    # the case has teeth: one ungrouped matcher over the 13 lanes reports cross-label pairs
    everything = capi.CrossMatcher(13, 300, min_len, t)
    everything.feed([x if len(x) else None for x in lanes])
    everything.finish()
    crossing = [pairs_of(13)[prob] for prob in by_pair(everything.runs())]
    assert sum(1 for a, b in crossing if TWO_SEASONS[a] != TWO_SEASONS[b]) >= 8
    for name, schedule in two_season_cuttings(p, lanes):
        got, stats = stream(lanes, TWO_SEASONS, 0, schedule, t, [300], [min_len])
        assert got == want, name
        assert stats[2] == live_cells(lanes, TWO_SEASONS, 0), name


# ---- 2. two regions, to results ------------------------------------------------------------------------------------------------------
def test_two_regions_go_straight_into_the_grouped_results():
    """Labels 0 and 0xFFFFFFFF and one video alone; the members of a group are not adjacent; the regions have capacities and
    min_len of their own.  The complete list is what needle_hip_comparator_results_from_runs_grouped takes."""
    labels = [0, 0xFFFFFFFF, 0, 5, 0xFFFFFFFF, 0]
    rng = np.random.default_rng(21)
    rows = random_rows(rng, [400 + 13 * v for v in range(len(labels))], regions=2)
    rows = [[video[0], video[1][:300 + 9 * v].copy()] for v, video in enumerate(rows)]
    for label in (0, 0xFFFFFFFF):
        for r in range(2):
            seg = rand_hashes(rng, 120 - 20 * r)
            for k, v in enumerate(v for v, g in enumerate(labels) if g == label):
                rows[v][r][8 + 11 * k + 3 * r: 8 + 11 * k + 3 * r + len(seg)] = seg ^ _masks([2] * len(seg), rng, 0)
    for r in range(2):                                                           # a longer segment across the labels, behind the groups' own
        cross = rand_hashes(rng, 130)
        for v in (0, 1, 3):
            rows[v][r][160:290] = cross
    videos = Videos(rows, even_timestamps(rows))
    cmp = capi.Comparator(videos.paths, include_endings=True, hash_match_threshold=10, min_opening_duration=10, min_ending_duration=20)
    min_len = [M.min_len_for(10), M.min_len_for(20)]
    max_items = [max(len(v[0]) for v in rows), max(len(v[1]) for v in rows)]
    assert max_items[0] != max_items[1] and min_len[0] != min_len[1]
    flat = [row for video in rows for row in video]
    want = oracle_live(flat, labels, 0, 10, min_len, 2)
    assert any(prob % 2 for prob in want) and any(prob % 2 == 0 for prob in want)
    lens = [len(x) for x in flat]
    rng = np.random.default_rng(5)
    schedule = random_schedule([chunks_from_cuts(set(rng.choice(np.arange(1, x), size=6, replace=False).tolist()), x) for x in lens], rng)
    m = new(flat, labels, 0, max_items, min_len, 10)
    feed(m, flat, schedule)
    m.finish()
    assert by_pair(m.runs()) == want
    got = _as(cmp.results_from_runs_grouped(videos.c, labels, m.runs()))
    assert got == _as(cmp.run_with_frame_hashes(videos.c, groups=labels))
    assert got[3] is None and all(got[v] is not None and got[v][0] is not None and got[v][1] is not None for v in (0, 1, 2, 4, 5))
    assert got != _as(cmp.run_with_frame_hashes(videos.c))                       # the segment across the labels wins ungrouped


# ---- 3. residents ----------------------------------------------------------------------------------------------------------------------
RES_LABELS = [1, 2, 9, 1, 2]                                                     # no arriving video has label 9
ARR_LABELS = [1, 2, 7, 2, 7, 3]                                                  # 7: no resident has it; 3: alone in its group


def library():
    rng = np.random.default_rng(33)
    rows = [rand_hashes(rng, n) for n in (60, 80, 70, 90, 50, 100, 110, 95, 120, 105, 40)]
    copy = lambda a, ra, b, cb, n: rows[b].__setitem__(slice(cb, cb + n), rows[a][ra: ra + n] ^ _masks([3] * n, rng, 0))
    copy(0, 10, 5, 20, 25)                                                       # label 1: resident 0 -> arriving 5
    copy(3, 90 - 20, 5, 60, 20)                                                  # ... and a run into resident 3's LAST row
    copy(1, 5, 6, 10, 30)                                                        # label 2: residents 1, 4 -> arriving 6, 8
    copy(4, 50 - 15, 8, 100, 15)                                                 # ... into resident 4's last row, lane 8's columns 100 ..
    copy(4, 5, 6, 96, 14)                                                        # ... into lane 6's last column
    copy(1, 45, 8, 75, 20)
    copy(6, 50, 8, 30, 40)                                                       # ... arriving 6 -> arriving 8
    copy(7, 10, 9, 15, 35)                                                       # label 7: arriving 7 -> arriving 9
    copy(2, 5, 5, 5, 12)                                                         # across labels: the resident nobody arrives for
    copy(0, 30, 6, 70, 25)                                                       # ... resident of 1 into arriving of 2
    copy(5, 40, 7, 60, 25)                                                       # ... arriving of 1 into arriving of 7
    copy(0, 0, 3, 0, 30)                                                         # resident - resident, same label
    copy(8, 0, 10, 5, 30)                                                        # into the video alone in its group
    return rows


def test_residents_over_three_labels():
    rows, labels, k, t, min_len = library(), RES_LABELS + ARR_LABELS, 5, 10, 8
    live = G.live_pairs(labels, k)
    assert sorted(live) == [(0, 5), (1, 6), (1, 8), (3, 5), (4, 6), (4, 8), (6, 8), (7, 9)]
    want = oracle_live(rows, labels, k, t, [min_len])
    assert sorted(want) == sorted(live.values()), "every live pair holds a planted run"
    lens = [len(x) for x in rows[k:]]
    rng = np.random.default_rng(6)
    ragged = random_schedule([chunks_from_cuts(set(rng.choice(np.arange(1, x), size=5, replace=False).tolist()), x) for x in lens], rng)
    for name, schedule in (("one feed", one_feed(rows[k:])), ("one item per feed", one_item_per_feed(lens)),
                           ("whole lanes, reversed", whole_lanes(lens, reversed(range(len(lens))))), ("ragged", ragged)):
        got, stats = stream(rows, labels, k, schedule, t, [120], [min_len])
        assert got == want, name                                                 # (no resident-resident, no cross-label problem)
        assert stats[2] == live_cells(rows, labels, k), name
    # without the resident nobody arrives for: the same state, the same runs under ids that shifted
    fewer_rows, fewer = rows[:2] + rows[3:], labels[:2] + labels[3:]
    sb = capi.CrossMatcher.state_bytes_grouped
    assert sb(labels[k:], [120], [len(x) for x in rows[:k]], labels[:k]) == sb(fewer[4:], [120], [len(x) for x in fewer_rows[:4]], fewer[:4])
    got, stats_fewer = stream(fewer_rows, fewer, 4, one_feed(fewer_rows[4:]), t, [120], [min_len])
    shifted = G.live_pairs(fewer, 4)
    assert got == {shifted[(a - (a > 2), b - 1)]: want[pid] for (a, b), pid in live.items()}
    assert stats_fewer[2] == stats[2] and stats_fewer[3] == stats[3] - 16        # one resident table entry


def test_a_run_into_a_residents_last_row_waits_for_its_lane():
    rows, labels, k, t, min_len = library(), RES_LABELS + ARR_LABELS, 5, 10, 8
    live = G.live_pairs(labels, k)
    want = oracle_live(rows, labels, k, t, [min_len])
    p35, p48 = live[(3, 5)], live[(4, 8)]
    last35 = [r for r in want[p35] if r[0] == len(rows[3]) - 1]
    last48 = [r for r in want[p48] if r[0] == len(rows[4]) - 1]
    assert last35 and last48
    m = new(rows, labels, k, [120], [min_len], t)
    m.feed(rows[k:])                                                             # everything is there, nothing is finished
    held = lambda prob, row: [r for r in by_pair(m.runs()).get(prob, []) if r[0] == len(rows[row]) - 1]
    assert not held(p35, 3) and not held(p48, 4)
    closed = by_pair(m.runs())
    assert closed[live[(0, 5)]] == want[live[(0, 5)]]                            # a run that cells broke is there already
    m.finish([1, 2, 4, 5])                                                       # lanes of videos 6, 7, 9, 10
    assert not held(p35, 3) and not held(p48, 4)
    m.finish([3])                                                                # video 8
    assert held(p48, 4) == last48 and not held(p35, 3)
    m.finish([0])                                                                # video 5
    assert held(p35, 3) == last35
    assert m.ready()[1] and by_pair(m.runs()) == want


# ---- 4. stats ------------------------------------------------------------------------------------------------------------------------------
def test_launches_cells_and_state_bytes():
    rows, labels, k = library(), RES_LABELS + ARR_LABELS, 5
    m = new(rows, labels, k, [120], [8], 10)
    live = G.live_pairs(labels, k)
    sb = capi.CrossMatcher.state_bytes_grouped(labels[k:], [120], [len(x) for x in rows[:k]], labels[:k])
    live_res = [(a, b) for a, b in live if a < k]
    assert sb == 2 * 4 * 120 * 2 + 6 * 120 * 4 + sum(2 * len(rows[a]) * 2 for a, b in live_res) + sum(len(rows[a]) * 4 for a in (0, 1, 3, 4))
    assert m.stats()[3] == sb + 24 * len(live) + 16 * k + SLAB
    assert sb < capi.CrossMatcher.state_bytes(6, [120], [len(x) for x in rows[:k]])   # the ungrouped formula for the same lanes
    rounds, fed = 0, [0] * 6
    for step in range(12):
        was = m.stats()
        chunk = [rows[k + q][fed[q]: fed[q] + 7] if (step + q) % 3 else None for q in range(6)]
        m.feed(chunk)
        for q in range(6):
            fed[q] += 0 if chunk[q] is None else len(chunk[q])
        rounds += 1
        now = m.stats()
        assert now[1] - was[1] == 3 and now[1] == 3 * rounds and now[3] == was[3]
        x = [max(len(r) - 1, 0) for r in rows[:k]] + [max(f - 1, 0) for f in fed]
        assert now[2] == sum(x[a] * x[b] for a, b in live), step
    was = m.stats()
    m.feed([None] * 6)                                                           # nothing: no round
    assert m.stats() == was
    m.finish([2])                                                                # a round without data adds no cells
    assert m.stats()[1] == 3 * (rounds + 1) and m.stats()[2] == was[2]
    # nobody has a partner: still three launches a round, no cells, no run
    lonely = capi.CrossMatcher.with_groups([1, 2, 3], [50], [2], 10)
    lonely.feed([rows[0][:40]] * 3)
    lonely.finish()
    assert lonely.stats()[:3] == (1, 6, 0) and lonely.ready() == (0, True)
    assert lonely.stats()[3] == 3 * 50 * 4 + SLAB == capi.CrossMatcher.state_bytes_grouped([1, 2, 3], [50]) + SLAB


# ---- 5. the 32-bit state ---------------------------------------------------------------------------------------------------------------------
def test_a_lane_of_65540_items_takes_the_32_bit_state():
    rng = np.random.default_rng(23)
    long_lane, partner, third, fourth = rand_hashes(rng, 65540), rand_hashes(rng, 48), rand_hashes(rng, 60), rand_hashes(rng, 44)
    partner[5:45] = long_lane[65500:65540] ^ _masks([1] * 40, rng, 0)            # a run into item 65 539: the long lane's last
    fourth[2:32] = third[20:50] ^ _masks([1] * 30, rng, 0)
    third[0:20] = long_lane[100:120]                                             # across the labels
    rows, labels = [long_lane, third, partner, fourth], [8, 4, 8, 4]
    want = oracle_live(rows, labels, 0, 9, [5])
    ids = G.live_pairs(labels, 0)
    assert sorted(want) == [ids[(0, 2)], ids[(1, 3)]] == [0, 1]
    assert any(r[:2] == (65539, 44) and r[2] >= 40 for r in want[0])
    sb = capi.CrossMatcher.state_bytes_grouped(labels, [65540])
    assert sb == 2 * 4 * 65540 * 4 + 4 * 65540 * 4 and capi.CrossMatcher.state_bytes_grouped(labels, [65535]) == 2 * 4 * 65535 * 2 + 4 * 65535 * 4
    schedule = [[(0, 30000), (0, 30), None, None], [(30000, 65000), None, (0, 20), (0, 44)], [(65000, 65540), (30, 60), (20, 48), None]]
    got, stats = stream(rows, labels, 0, schedule, 9, [65540], [5])
    assert got == want
    assert stats[2] == live_cells(rows, labels, 0) and stats[3] == sb + 24 * 2 + SLAB


# ---- 6. bounds -------------------------------------------------------------------------------------------------------------------------------
def test_bounds_are_on_the_live_problems():
    """300 residents and 256 arriving videos, max_items 8: 64 shows of four arrive, each with one resident; 236 residents are
    of shows that do not arrive.  640 live pairs where the ungrouped numbering has 109 440."""
    rng = np.random.default_rng(24)
    res_labels, arr_labels = list(range(300)), [t // 4 for t in range(256)]
    labels = res_labels + arr_labels
    rows = [rand_hashes(rng, int(n)) for n in rng.integers(3, 9, 556)]
    base = rand_hashes(rng, 8)
    for v in range(0, 556, 3):                                                   # a third of all videos hold a common stretch
        rows[v][:len(rows[v])] = base[:len(rows[v])]
    live = G.live_pairs(labels, 300)
    assert len(live) == 256 + 64 * 6
    want = oracle_live(rows, labels, 300, 10, [2])
    assert len(want) >= 40
    schedule = [[(0, 2) for _ in range(256)], [(2, len(x)) for x in rows[300:]]]
    got, stats = stream(rows, labels, 300, schedule, 10, [8], [2])
    assert got == want
    assert stats[1] == 9 and stats[2] == live_cells(rows, labels, 300)
    with pytest.raises(capi.NeedleError) as e:                                   # the same without labels: the existing entry point
        capi.CrossMatcher.with_resident(rows[:300], 256, [8], [2], 10)
    assert e.value.code == INVALID and "live problems" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:                                   # 256 residents of one label and all 256 arriving: 65 536 + 32 640
        capi.CrossMatcher.with_groups([0] * 256, [8], [2], 10, resident=rows[:256], resident_groups=[0] * 256)
    assert e.value.code == INVALID and "65 535 live problems" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:                                   # exactly 65 536: 65 535 residents of one arriving video, and one arriving pair
        capi.CrossMatcher.with_groups([0, 1, 1], [8], [2], 10, resident=[rows[0]] * 65535, resident_groups=[0] * 65535)
    assert e.value.code == INVALID and "65 535 live problems" in str(e.value)


# ---- 7. one label is the object without labels ---------------------------------------------------------------------------------------------
def test_one_label_is_the_object_without_labels():
    """One plan (cross_pairs.h) lays out both: the same data through an object made without labels (the walk finds its problems
    by arithmetic) and one made with a single label (the walk reads the uploaded table).  Two residents, one with a row of one
    hash; three arriving videos; two regions with capacities and min_len of their own; ragged feeds; one lane finished early; a
    run into resident 0's last row that arrives long before its lane finishes.  After every step the two hold the same runs
    under the same problems, and the same feeds, launches and cells; the state differs by the table: 24 bytes a live problem."""
    rng = np.random.default_rng(41)
    k, videos, max_items, min_len, t = 2, 3, [48, 20], [3, 2], 10
    lens = [30, 14, 1, 9] + [48, 20, 40, 17, 33, 20]                              # rows video * 2 + region, residents first
    rows = [rand_hashes(rng, n) for n in lens]
    copy = lambda a, ra, b, cb, n: rows[b].__setitem__(slice(cb, cb + n), rows[a][ra: ra + n] ^ _masks([2] * n, rng, 0))
    copy(0, 30 - 10, 4, 5, 10)                                                   # region 0: into resident 0's LAST row, lane 0's items 5 .. 14
    copy(0, 3, 6, 20, 12)                                                        # ... resident 0 -> arriving 1
    copy(4, 30, 8, 10, 15)                                                       # ... arriving 0 -> arriving 2
    copy(1, 14 - 6, 7, 2, 6)                                                     # region 1: into resident 0's last row, lane 3
    copy(3, 1, 9, 11, 7)                                                         # ... resident 1 -> arriving 2
    copy(5, 4, 7, 9, 8)                                                          # ... arriving 0 -> arriving 1
    labels = [7] * (k + videos)
    live = G.live_pairs(labels, k)
    assert list(live.values()) == [pair_index(a, b, k + videos) for a, b in live] and len(live) == 9   # one label: the comparator's ids
    want = oracle_live(rows, labels, k, t, min_len, 2)
    last_row = {prob: [r for r in runs if r[0] == lens[0 + prob % 2] - 1] for prob, runs in want.items()
                if prob // 2 in (live[(0, 2)], live[(0, 3)])}
    assert last_row[live[(0, 2)] * 2] and last_row[live[(0, 3)] * 2 + 1] and len(want) >= 6
    plain = capi.CrossMatcher.with_resident(rows[:4], videos, max_items, min_len, t)
    one = new(rows, labels, k, max_items, min_len, t)
    assert plain.groups is None
    lanes = rows[4:]
    steps = [[(0, 20), (0, 9), None, (0, 17), (0, 1), None],                     # lane 3 whole; lane 4 one item: no cells yet
             ("finish", [3]),                                                    # ... and finished early
             [(20, 21), None, (0, 33), None, (1, 30), (0, 20)],
             [(21, 48), (9, 20), (33, 40), None, None, None],
             ("finish", [1, 2]),
             [None, None, None, None, (30, 33), None]]
    held = lambda m, prob: [r for r in by_pair(m.runs()).get(prob, []) if r in last_row[prob]]
    for n, step in enumerate(steps):
        for m in (plain, one):
            if step[0] == "finish":
                m.finish(step[1])
            else:
                m.feed([None if part is None else lanes[q][part[0]: part[1]] for q, part in enumerate(step)])
        assert by_pair(plain.runs()) == by_pair(one.runs()) and len(plain.runs()) == len(one.runs()), n
        assert plain.stats()[:3] == one.stats()[:3], n
        assert not held(one, live[(0, 2)] * 2), n                                # lane 0 is not finished: its run into the last row waits
        assert held(one, live[(0, 3)] * 2 + 1) == ([] if n == 0 else last_row[live[(0, 3)] * 2 + 1]), n   # lane 3's came with its finish
    for m in (plain, one):
        m.finish()
        assert m.ready()[1] is True
    assert by_pair(plain.runs()) == by_pair(one.runs()) == want
    assert plain.stats()[:3] == one.stats()[:3] and plain.stats()[2] == live_cells(rows, labels, k, 2)
    assert one.stats()[3] - plain.stats()[3] == 24 * len(live) * 2
    assert plain.stats()[3] == capi.CrossMatcher.state_bytes(videos, max_items, lens[:4]) + 16 * 4 + SLAB


# ---- 9. the existing objects launch what they launched ---------------------------------------------------------------------------------------
def test_a_plain_cross_matcher_launches_what_it_launched():
    rng = np.random.default_rng(25)
    rows = [rand_hashes(rng, 90) for _ in range(5)]

    def plain():
        m = capi.CrossMatcher.with_resident(rows[:2], 3, [100], [4], 10)
        for at in range(0, 90, 30):
            m.feed([x[at: at + 30] for x in rows[2:]])
        m.finish()
        return by_pair(m.runs())

    def grouped():
        got, _ = stream(rows, [1, 2, 1, 2, 1], 2, one_feed(rows[2:]), 10, [100], [4])
        return got

    first = []
    before = timed(lambda: first.append(plain()))
    assert grouped() == oracle_live(rows, [1, 2, 1, 2, 1], 2, 10, [4])
    second = []
    after = timed(lambda: second.append(plain()))
    assert before == after == {"crossmatch_land": 4, "crossmatch_walk": 4, "crossmatch_simhash": 4}
    assert first == second
    assert timed(grouped) == {"crossmatch_land": 2, "crossmatch_walk": 2, "crossmatch_simhash": 2}
