"""-m gpu: several shows' seasons streamed into a grouped index (needle_hip_index_crossmatcher_new_grouped,
needle_hip_index_add_matched_grouped; csrc/index.cpp, the grouped ingest in csrc/index_store.hip, the grouped cross-matcher in
csrc/crossmatch.hip).  The reference of every positive test is a twin index that received the same videos through
add(groups=...), checked against the oracle per show as tests/test_gpu_index_grouped.py checks it: results, evidence, store
sizes, pairs_searched and groups() must agree while pairs_scanned says that nothing was scanned.  What can go wrong is the
numbering (the grouped id over all K + k videos against the store's append-stable ids), which rows are gathered, the runs the
scan's problems exclude, and what a refused call leaves behind."""
import ctypes as C

import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests import best_match_model as M
from tests.test_gpu_feeder_formats import timed
from tests.test_gpu_grouped import HD, Videos, _as, even_timestamps, members_of, random_rows
from tests.test_gpu_index_grouped import A, B, C2, LABELS12, Live, _library_of_four_groups, _new, _plant_extra
from tests.test_gpu_index_matched import _copy_of, _feed_ragged, _lanes
from tests.test_gpu_library_rates import windows

pytestmark = pytest.mark.gpu
INVALID = capi.ERROR_NAMES.index("InvalidArgument")
NEW_SHOW = 4242


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _season(index, fhs, labels, min_len, regions=1, feed=_feed_ragged):
    """A complete grouped matcher made from `index` that has been fed the videos `fhs` under `labels`."""
    rows = _lanes(fhs, regions)
    max_items = [max(2, max(len(x) for x in rows[r::regions])) for r in range(regions)]
    m = index.crossmatcher(len(fhs), max_items, min_len, groups=labels)
    assert m.resident == len(index) and m.shape() == (len(fhs), regions)
    assert m.groups.tolist() == index.groups() + list(labels)
    feed(m, rows)
    return m


def _state(index):
    return len(index), index.groups(), _as(index.results()), index.pairs_searched(), index.pairs_scanned(), index.store_sizes()


def _same_evidence(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for name in ("opening", "ending"):
            assert M.same_evidence(getattr(g, name), getattr(w, name)), (name, g, w)


def _agree(streamed, twin, scanned_before):
    """After add_matched on `streamed` and add(groups=...) of the same videos on the twin (a Live, checked against the oracle)."""
    assert _as(streamed.results()) == _as(twin.index.results()) == twin.expect()
    _same_evidence(streamed.evidence(), twin.index.evidence())
    assert streamed.store_sizes() == twin.index.store_sizes()
    assert streamed.pairs_searched() == twin.index.pairs_searched()
    assert streamed.groups() == twin.index.groups() == twin.labels
    assert streamed.pairs_scanned() == (scanned_before, 0)


def _library(extra_labels):
    rows, segs = _library_of_four_groups(extra=len(extra_labels))
    for k, label in enumerate(extra_labels):
        if label in segs:
            _plant_extra(rows, segs, 12 + k, label, 5 + k)
    return rows, LABELS12 + list(extra_labels)


# ---- 7. the index route ----------------------------------------------------------------------------------------------------------------
def test_five_videos_of_three_shows_join_a_grouped_index(monkeypatch):
    """A grouped index of 8 (four groups); then two more of show A, two of show B and one of a new show, streamed.  Show C2 and
    the video alone do not arrive: their rows are not gathered and their results stay."""
    rows, labels = _library([B, NEW_SHOW, NEW_SHOW])
    pool = Videos(rows, even_timestamps(rows))
    twin = Live(pool, labels, monkeypatch, min_s=20)
    twin.add(list(range(8)))
    streamed = capi.Index(twin.cmp, grouped=True)
    streamed.add(pool.c[:8], groups=labels[:8])
    arriving = [8, 10, 11, 12, 13]
    assert [labels[v] for v in arriving] == [A, B, A, B, NEW_SHOW]
    fhs, groups = [pool.c[v] for v in arriving], [labels[v] for v in arriving]
    before = _as(streamed.results())
    scanned = streamed.pairs_scanned()[0]
    m = _season(streamed, fhs, groups, [M.min_len_for(20)])
    assert m.ready()[0] >= 8
    live = sum(labels[:8].count(g) for g in groups) + 2                          # each with its show's residents; (8, 11) and (10, 12)
    assert m.stats()[3] - (32 + 4096 * 24) - 16 * 8 - 24 * live == capi.CrossMatcher.state_bytes_grouped(
        groups, m.max_items, [len(pool.rows[v][0]) for v in range(8)], labels[:8])
    streamed.add_matched(m, fhs)
    twin.add(arriving)
    _agree(streamed, twin, scanned)
    assert streamed.pairs_searched()[1] == live == 3 + 3 + 4 + 4 + 0             # ranks: A 3, B 3, A 4, B 4, the new show 0
    got = _as(streamed.results())
    assert got[12] is None and all(got[v] is not None and got[v][0] is not None for v in range(13) if v not in (3, 6, 12))
    assert [got[v] for v in (3, 6)] == [before[v] for v in (3, 6)]               # C2's only member so far, and the video alone
    # a second season from the grown index: C2's second member and the new show's second
    more, more_labels = [pool.c[9], pool.c[14]], [C2, NEW_SHOW]
    scanned = streamed.pairs_scanned()[0]
    streamed.add_matched(_season(streamed, more, more_labels, [M.min_len_for(20)]), more)
    twin.add([9, 14])
    _agree(streamed, twin, scanned)
    assert streamed.pairs_searched()[1] == 2


def test_a_first_season_of_two_shows_into_an_empty_grouped_index(monkeypatch):
    rows, labels = _library([])
    pool = Videos(rows, even_timestamps(rows))
    twin = Live(pool, labels, monkeypatch, min_s=20)
    streamed = capi.Index(twin.cmp, grouped=True)
    first = [0, 1, 2, 4, 5]                                                      # A B A B A
    fhs, groups = [pool.c[v] for v in first], [labels[v] for v in first]
    m = _season(streamed, fhs, groups, [M.min_len_for(20)])
    assert m.resident == 0 and m.ready()[0] >= 4
    # without residents the list is what results_from_runs_grouped takes
    assert _as(twin.cmp.results_from_runs_grouped(fhs, groups, m.runs())) == _as(twin.cmp.run_with_frame_hashes(fhs, groups=groups))
    streamed.add_matched(m, fhs)
    twin.add(first)
    _agree(streamed, twin, 0)
    assert streamed.pairs_scanned() == (0, 0) and streamed.pairs_searched() == (4, 4)


def test_endings_and_a_video_without_ending_data(monkeypatch):
    """Two regions of unequal lengths.  An arriving video without ending data is accepted alone in its show (its ending lane is
    finished empty) and refused, in add's words, where its show has another member."""
    labels = [1, 2, 1, 3, 2, 1, 2, 3, 1]
    rng = np.random.default_rng(15)
    rows = random_rows(rng, [380 + 17 * v for v in range(len(labels))], regions=2)
    rows = [[video[0], video[1][:300 + 11 * v].copy()] for v, video in enumerate(rows)]
    for m in members_of(labels):
        for r in range(2):
            seg = _new(rng, 110 + 12 * r)
            for k, v in enumerate(m):
                flips = (np.uint32(1) << rng.integers(0, 32, len(seg)).astype(np.uint32)) * (rng.random(len(seg)) < 0.3)
                rows[v][r][10 + 11 * k + 5 * r: 10 + 11 * k + 5 * r + len(seg)] = seg ^ flips.astype(np.uint32)
    for r in range(2):                                                           # across the shows
        cross = _new(rng, 200)
        for v in (0, 1, 3, 6):
            rows[v][r][170:290] = cross[:120]
    ts = even_timestamps(rows)
    pool = Videos(rows, ts)
    opening = list(zip(rows[4][0].tolist(), ts[4][0]))                           # video 9: video 4's opening and no ending data at all
    pool.c.append(capi.FrameHashes.new(opening, [], HD))
    pool.o.append(O.FrameHashes(opening, [], HD, ""))
    pool.rows.append([rows[4][0], np.zeros(0, dtype=np.uint32)])
    twin = Live(pool, labels + [4040], monkeypatch, min_s=15, padding=0.5, evidence=False)
    twin.add([0, 1, 2, 3])
    streamed = capi.Index(twin.cmp, grouped=True)
    streamed.add(pool.c[:4], groups=labels[:4])
    arriving = [4, 5, 6, 7, 8, 9]
    fhs, groups = [pool.c[v] for v in arriving], [twin.pool_labels[v] for v in arriving]
    min_len = [M.min_len_for(15)] * 2
    # ... in a show that has other members: refused as add_grouped refuses it, the index as it was
    was = _state(streamed)
    bad = _season(streamed, fhs, groups[:5] + [2], min_len, regions=2)
    with pytest.raises(capi.NeedleError, match="no ending hash data present"):
        streamed.add_matched(bad, fhs)
    assert _state(streamed) == was
    scanned = streamed.pairs_scanned()[0]
    m = _season(streamed, fhs, groups, min_len, regions=2)
    assert m.lane(11) == (0, True) and any(int(x["problem"]) % 2 for x in m.runs())
    streamed.add_matched(m, fhs)
    twin.add(arriving)
    _agree(streamed, twin, scanned)
    got = _as(streamed.results())
    assert got[9] is None and all(r is not None and r[0] is not None for r in got[:9]) and any(r[1] is not None for r in got[:9])


def test_from_pcm_through_one_feeder_into_a_grouped_index():
    """Five episodes that all hold the same intro, as two shows: one feeder, one grouped cross-matcher, one append."""
    eps = synth.make_library(5, 90.0, 20.0, 0.0)
    names = [f"/tmp/needle_grouped_ep{k}.wav" for k in range(5)]
    labels = [1, 2, 1, 2, 1]
    full = capi.Analyzer.from_files(names).run_pcm([e.pcm for e in eps], channels=1)
    cmp = capi.Comparator(names, min_opening_duration=10)
    want = _as(cmp.run_with_frame_hashes(full, groups=labels))
    assert all(r is not None and r[0] is not None for r in want)
    index = capi.Index(cmp, grouped=True)
    index.add(full[:2], groups=labels[:2])
    opening = [e.pcm[: windows(len(e.pcm), 1, 11025, endings=False)[0][1]] for e in eps[2:]]
    longest = max(capi.feeder_num_ready(len(x), 11025, 1, 2, True) for x in opening)
    f = capi.Feeder(3, 1, 11025, capi.SAMPLE_S16, 2)
    m = index.crossmatcher(3, [longest], [30], groups=labels[2:])
    pos, step = [0, 0, 0], 0
    while not m.ready()[1]:
        chunk = []
        for q, x in enumerate(opening):
            take = 0 if (step + q) % 3 == 0 else 3000 + 1700 * q                 # a few thousand samples, out of step
            chunk.append(x[pos[q]: pos[q] + take] if take and pos[q] < len(x) else None)
            pos[q] = min(len(x), pos[q] + take)
        f.feed(chunk)
        ended = [q for q in range(3) if pos[q] == len(opening[q]) and not f.ready(q)[2]]
        if ended:
            f.finish(ended)
        m.feed_from_feeder(f)
        step += 1
    assert m.ready()[0] >= 1
    streamed = [f.frame_hashes(q) for q in range(3)]
    index.add_matched(m, streamed)
    assert _as(index.results()) == want
    assert index.groups() == labels and index.pairs_scanned() == (0, 0) and index.pairs_searched() == (4, 4)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def _refused(index, matcher, fhs, words):
    before = _state(index)
    with pytest.raises(capi.NeedleError) as e:
        index.add_matched(matcher, fhs)
    assert e.value.code == INVALID and words in str(e.value), str(e.value)
    assert _state(index) == before, "a refused add_matched leaves the index as it was"


def test_refusals_leave_the_grouped_index_as_it_was(monkeypatch):
    rows, labels = _library([])
    pool = Videos(rows, even_timestamps(rows))
    cmp, _ = pool.comparators(min_s=20)
    low = M.min_len_for(20)
    index, other, plain = capi.Index(cmp, grouped=True), capi.Index(cmp, grouped=True), capi.Index(cmp)
    for ix in (index, other):
        ix.add(pool.c[:8], groups=labels[:8])
    plain.add(pool.c[:8])
    new, groups = [pool.c[8], pool.c[10], pool.c[11]], [labels[8], labels[10], labels[11]]      # A B A
    lanes = _lanes(new, 1)
    cap = [max(len(x) for x in lanes)]

    _refused(index, _season(other, new, groups, [low]), new, "not created from this index")   # foreign
    loose = capi.CrossMatcher.with_groups(groups, cap, [low], 10, resident=_lanes(pool.c[:8], 1), resident_groups=labels[:8])
    _feed_ragged(loose, lanes)
    _refused(index, loose, new, "not created from this index")
    from_plain = plain.crossmatcher(3, cap, [low])                               # an ungrouped matcher, made from a plain index
    _feed_ragged(from_plain, lanes)
    _refused(index, from_plain, new, "no streamed routes")                       # ... goes to the old entry point, refused in the old words
    from_plain._grouped = True                                                   # ... and to the new one, not this index's
    _refused(index, from_plain, new, "not created from this index")
    from_plain._grouped = False
    good = _season(index, new, groups, [low])
    was = (len(plain), _as(plain.results()), plain.pairs_searched())
    with pytest.raises(capi.NeedleError, match="not a grouped index"):           # a plain index has no grouped route
        capi.check(capi.lib().needle_hip_index_add_matched_grouped(plain._h, good._h, (C.c_void_p * 3)(*[f._h for f in new]), 3))
    with pytest.raises(capi.NeedleError, match="not a grouped index"):
        plain.crossmatcher(3, cap, [low], groups=groups)
    assert (len(plain), _as(plain.results()), plain.pairs_searched()) == was
    half = index.crossmatcher(3, cap, [low], groups=groups)
    half.feed([lanes[0], lanes[1][:100], None])
    half.finish([0])
    _refused(index, half, new, "not complete")
    _refused(index, good, new[:2], "number of videos")
    _refused(index, good, [new[0], new[1], _copy_of(new[2], drop=1)], "not as long")
    for video, word in ((0, 0), (2, len(lanes[2]) - 1), (1, 150)):               # ONE hash word differs from the lane's history
        fhs = list(new)
        fhs[video] = _copy_of(new[video], flip=word)
        _refused(index, good, fhs, "hashes differ")
    _refused(index, _season(index, new, groups, [low + 1]), new, "min_len")
    # the old four entry points are refused in their old words
    for call in (lambda: index.crossmatcher(3, cap, [low]), lambda: index.matcher(3)):
        before = _state(index)
        with pytest.raises(capi.NeedleError, match="a grouped index has no streamed routes"):
            call()
        assert _state(index) == before
    good._grouped = False
    _refused(index, good, new, "a grouped index has no streamed routes")
    good._grouped = True
    before = _state(index)
    with pytest.raises(capi.NeedleError, match="a grouped index has no streamed routes"):
        index.add_streamed(plain.matcher(1), None, new[:1])
    assert _state(index) == before
    # every one of them left `good` usable ...
    twin = Live(pool, labels, monkeypatch, min_s=20, evidence=False)
    twin.add(list(range(8)))
    scanned = index.pairs_scanned()[0]
    index.add_matched(good, new)
    twin.add([8, 10, 11])
    _agree(index, twin, scanned)
    # ... and consumed: stale after its own append, and after any other change
    _refused(index, good, new, "changed since")
    stale = index.crossmatcher(1, cap, [low], groups=[C2])
    index.remove([0])
    _refused(index, stale, [pool.c[9]], "changed since")


# ---- 9. the plain route launches what it launched ---------------------------------------------------------------------------------------
def test_a_plain_streamed_append_launches_what_it_launched(monkeypatch):
    rows, labels = _library([])
    pool = Videos(rows, even_timestamps(rows))
    cmp, _ = pool.comparators(min_s=20)
    low = M.min_len_for(20)

    def plain_route(results):
        ix = capi.Index(cmp)
        ix.add(pool.c[:8])
        lanes = _lanes(pool.c[8:], 1)
        m = ix.crossmatcher(4, [max(len(x) for x in lanes)], [low])
        m.feed(lanes)
        m.finish()
        ix.add_matched(m, pool.c[8:])
        results.append(_as(ix.results()))

    first, second = [], []
    before = timed(lambda: plain_route(first))
    grouped = capi.Index(cmp, grouped=True)
    grouped.add(pool.c[:8], groups=labels[:8])
    grouped.add_matched(_season(grouped, pool.c[8:], labels[8:], [low]), pool.c[8:])
    after = timed(lambda: plain_route(second))
    assert before == after and first == second
    assert before["crossmatch_walk"] >= 2 and before["index_ingest"] == 1 and before["crossmatch_gather_resident"] == 1
