"""-m gpu: a streamed season into an index of any size (needle_hip_index_matcher_new, needle_hip_index_add_streamed;
csrc/index.cpp, the ingest in csrc/index_store.hip, the regions and the gather in csrc/matcher.hip).  The resident x arriving
pairs come from a region-aware matcher made from the index, the arriving x arriving pairs from a cross-matcher without
residents.  The reference of every positive test is a twin index that received the same videos through plain `add` (and,
where the corpus is small, the oracle over the whole list): results, store sizes, pairs_searched must agree while
pairs_scanned says that nothing was scanned.  What can go wrong is the re-tagging of the two lists (source and lane to a
pair; an i-major pair over the k arriving videos to one over all), the runs the scan's problems exclude, and what a refused
call leaves behind.

One refusal of the contract has no test: "a run that does not lie inside its rows".  Both objects only report runs inside
what they were fed, and a row that differs from what was fed is refused first, so no sequence of public calls reaches it."""
import numpy as np
import pytest

from needle_amd import capi, synth
from tests.test_gpu_index import Corpus, _as, _planted, _segments
from tests.test_gpu_index_matched import _copy_of, _lanes, _min_len, _plant, _state
from tests.test_gpu_library_rates import windows

pytestmark = pytest.mark.gpu
INVALID, UNKNOWN = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("Unknown")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _feed_both(mt, cm, rows, sizes=(1, 37, 64, 5)):
    """Feeds both objects the same ragged chunks: lane i takes the sizes rotated by i, sits every fourth round out, then takes
    the rest in pieces of its own size, and is finished in the round its last item went in.  `cm` may be None."""
    pos, step = [0] * len(rows), 0
    while not all(mt.ready(i)[2] for i in range(len(rows))):
        chunk = []
        for i, x in enumerate(rows):
            take = 0 if (step + i) % 4 == 3 else sizes[(step + i) % len(sizes)] if step < 6 else 90 + 35 * i
            chunk.append(x[pos[i]: pos[i] + take] if take and pos[i] < len(x) else None)
            pos[i] = min(len(x), pos[i] + take)
        ended = [i for i, x in enumerate(rows) if pos[i] == len(x) and not mt.ready(i)[2]]
        for m in (mt, cm):
            if m is not None:
                m.feed(chunk)
                if ended:
                    m.finish(ended)
        step += 1
    assert [mt.ready(i)[1:] for i in range(len(rows))] == [(len(x), True) for x in rows]
    assert cm is None or (cm.ready()[1] and [cm.lane(i) for i in range(len(rows))] == [(len(x), True) for x in rows])


def _feed_whole(mt, cm, rows):
    for m in (mt, cm):
        if m is not None:
            m.feed(rows)
            m.finish()


def _season(index, fhs, min_len, regions, feed=_feed_both, cross=True):
    """A complete matcher made from `index` and the complete cross-matcher of the arriving pairs, both fed the videos `fhs`."""
    rows = _lanes(fhs, regions)
    mt = index.matcher(len(fhs))
    assert (mt.lanes, mt.regions, mt.num_sources) == (len(fhs) * regions, regions, len(index) * regions)
    cm = None
    if cross:
        cm = capi.CrossMatcher.with_regions(len(fhs), [max(len(x) for x in rows[r::regions]) for r in range(regions)], min_len, index.threshold)
        assert cm.resident == 0
    feed(mt, cm, rows)
    return mt, cm


def _agree(streamed, plain, resident, want=None):
    """After an add_streamed on `streamed` and the add of the same videos on `plain`."""
    got = _as(streamed.results())
    assert got == _as(plain.results())
    assert want is None or got == want, "add_streamed disagrees with the oracle"
    assert len(streamed) == len(plain) and streamed.store_sizes() == plain.store_sizes()
    assert streamed.pairs_searched() == plain.pairs_searched()
    assert streamed.pairs_scanned()[1] == 0 and plain.pairs_scanned()[1] == plain.pairs_searched()[1]
    assert any(r is not None and r[0] is not None for r in got[:resident]), "a resident video has an opening"
    assert any(r is not None and r[0] is not None for r in got[resident:]), "an arriving video has an opening"


def _corpus(seed=73):
    """8 videos with endings, every row of its own length: 3 known, 3 arriving, then one alone, then one through `add`.
    Planted in both regions: the shared segments of test_gpu_index (every pair holds one), a run into a resident row's last
    hash, one into a lane's last item, one from hash 0 on both sides, and one between two arriving videos only."""
    rng = np.random.default_rng(seed)
    lens = [[300, 333, 420, 371, 389, 312, 405, 350], [310, 420, 345, 398, 301, 417, 366, 322]]
    rows = _planted(rng, 8, 420, _segments(rng, lengths=(110, 80, 60), bases=(7, 150, 230)), endings=True)
    rows = [[h[:lens[r][v]].copy() for r, h in enumerate(video)] for v, video in enumerate(rows)]
    new = lambda n: rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    for r in range(2):
        n = lens[r]
        _plant(rows, new(70), [(1, r, n[1] - 70), (4, r, 100)], rng)             # ends on resident 1's last hash
        _plant(rows, new(90), [(2, r, 120), (5, r, n[5] - 90)], rng)             # ends on arriving 5's last item
        _plant(rows, new(64), [(0, r, 0), (3, r, 0), (6, r, 200)], rng)          # starts at hash 0 on both sides
        _plant(rows, new(75), [(3, r, 220), (5, r, 60)], rng)                    # arriving x arriving only
    corpus = Corpus(endings=True, min_s=10)
    for video in rows:
        corpus.add_rows(*video)
    return corpus


# ---- 1. equivalence with add ---------------------------------------------------------------------------------------------------
def test_a_season_joins_a_library_like_add():
    corpus = _corpus()
    low = [_min_len(10)] * 2
    streamed, plain = capi.Index(corpus.comparator()), capi.Index(corpus.comparator())
    for ix in (streamed, plain):
        ix.add(corpus.c[:2])
        ix.add(corpus.c[2:3])                                                    # two appends: arena offsets are not trivial
    new = corpus.c[3:6]
    mt, cm = _season(streamed, new, low, 2)
    per_lane = [mt.runs(i) for i in range(6)]
    assert all(len(x) for x in per_lane) and cm.ready()[0] >= 2
    assert all(int(p) % 2 == i % 2 and int(p) < 6 for i, x in enumerate(per_lane) for p in x["problem"]), "sources of the lane's region"
    before = streamed.pairs_scanned()
    streamed.add_streamed(mt, cm, new)
    plain.add(new)
    _agree(streamed, plain, 3, corpus.expect(6))
    assert streamed.pairs_scanned() == (before[0], 0) and streamed.pairs_searched()[1] == 3 * 3 + 3
    # one video alone: no arriving pair, no cross-matcher
    mt, _ = _season(streamed, corpus.c[6:7], low, 2, cross=False)
    streamed.add_streamed(mt, None, corpus.c[6:7])
    plain.add(corpus.c[6:7])
    _agree(streamed, plain, 6, corpus.expect(7))
    assert streamed.pairs_searched()[1] == 6
    # one further ordinary add on both
    for ix in (streamed, plain):
        ix.add(corpus.c[7:])
    assert _as(streamed.results()) == _as(plain.results()) == corpus.expect(8)
    assert streamed.store_sizes() == plain.store_sizes() and streamed.pairs_searched() == plain.pairs_searched()
    assert streamed.pairs_scanned()[0] < plain.pairs_scanned()[0] == plain.pairs_searched()[0]


def test_from_pcm_through_one_feeder_into_both_objects():
    """decoders -> feeder -> matcher and cross-matcher -> index, with endings: one feeder of videos x regions lanes feeds both,
    each from its own items_fed on."""
    known, arriving = 3, 3
    eps = synth.make_library(known + arriving, 90.0, 20.0, 15.0)
    names = [f"/tmp/needle_streamed_ep{k}.wav" for k in range(known + arriving)]
    full = capi.Analyzer.from_files(names).with_include_endings(True).run_pcm([e.pcm for e in eps], channels=1)
    cmp = capi.Comparator(names, include_endings=True, min_opening_duration=10, min_ending_duration=10)
    want = _as(cmp.run_with_frame_hashes(full))
    assert all(r is not None and r[0] is not None and r[1] is not None for r in want)
    streamed, plain = capi.Index(cmp), capi.Index(cmp)
    for ix in (streamed, plain):
        ix.add(full[:known])
    streams, seeks = [], []
    for e in eps[known:]:
        (o0, on), (e0, en, seek) = windows(len(e.pcm), 1, 11025)
        streams += [e.pcm[o0: o0 + on], e.pcm[e0: e0 + en]]
        seeks.append(seek)
    n = 2 * arriving
    cap = [max(capi.feeder_num_ready(len(streams[k]), 11025, 1, 2, True) for k in range(r, n, 2)) for r in range(2)]
    f = capi.Feeder(n, 1, 11025, capi.SAMPLE_S16, 2)
    mt = streamed.matcher(arriving)
    cm = capi.CrossMatcher.with_regions(arriving, cap, [30, 30], streamed.threshold)
    pos, step = [0] * n, 0
    while not cm.ready()[1]:
        chunk = []
        for k in range(n):
            take = 0 if (step + k) % 3 == 0 else 11025 // 2 + 900 * k            # the lanes out of step
            chunk.append(streams[k][pos[k]: pos[k] + take] if take and pos[k] < len(streams[k]) else None)
            pos[k] = min(len(streams[k]), pos[k] + take)
        f.feed(chunk)
        ended = [k for k in range(n) if pos[k] == len(streams[k]) and not f.ready(k)[2]]
        if ended:
            f.finish(ended)
        mt.feed_from_feeder(f)
        if step % 2 or all(f.ready(k)[2] for k in range(n)):                     # the cross-matcher takes every other round
            cm.feed_from_feeder(f)
        assert [mt.ready(k)[1:] for k in range(n)] == [(f.ready(k)[0], f.ready(k)[2]) for k in range(n)]
        step += 1
    fhs = [f.frame_hashes(2 * k, 2 * k + 1, seeks[k]) for k in range(arriving)]
    for got, ref in zip(fhs, full[known:]):
        assert got.opening_data()[0].tolist() == ref.opening_data()[0].tolist()
        assert got.ending_data()[0].tolist() == ref.ending_data()[0].tolist()
    streamed.add_streamed(mt, cm, fhs)
    plain.add(fhs)
    _agree(streamed, plain, known, want)


# ---- 2. beyond the cross-matcher's limit --------------------------------------------------------------------------------------
def test_a_season_beyond_the_cross_matchers_limit():
    """129 resident and 256 arriving videos, two regions: (129 x 256 + 256 x 255 / 2) x 2 = 131 328 live problems, which one
    cross-matcher refuses; the cross-matcher of the arriving pairs alone needs 32 640 x 2 = 65 280 and fits."""
    K, N, n_open, n_end = 129, 256, 40, 36
    rng = np.random.default_rng(79)
    new = lambda n: rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    rows = [[new(n_open), new(n_end)] for _ in range(K + N)]
    A, B = 1, 19                                                                 # two places for 16 hashes in a row
    for r, (a, at_a), (b, at_b) in ((0, (5, A), (K + 7, A)), (0, (0, A), (K, A)), (0, (K, B), (K + 255, A)), (0, (K + 254, A), (K + 255, B)),
                                    (1, (128, A), (K + 255, A)), (1, (K + 100, A), (K + 101, B)), (1, (64, B), (K + 128, A)),
                                    (1, (K, A), (K + 1, A))):
        _plant(rows, new(16), [(a, r, at_a), (b, r, at_b)], rng)
    corpus = Corpus(endings=True, min_s=1)
    for video in rows:
        corpus.add_rows(*video)
    low = _min_len(1)
    assert low == 5 and (K * N + N * (N - 1) // 2) * 2 == 131_328 > 65_535 >= N * (N - 1)
    streamed, plain = capi.Index(corpus.comparator()), capi.Index(corpus.comparator())
    for ix in (streamed, plain):
        ix.add(corpus.c[:K])
    with pytest.raises(capi.NeedleError) as e:                                   # the limit stays where it was, in today's words
        streamed.crossmatcher(N, [n_open, n_end], [low, low])
    assert e.value.code == INVALID and "live problems" in str(e.value)
    before = _state(streamed)
    mt, cm = _season(streamed, corpus.c[K:], [low, low], 2, feed=_feed_whole)
    assert mt.stats()[1] == 3 * 2 and _state(streamed) == before
    streamed.add_streamed(mt, cm, corpus.c[K:])
    plain.add(corpus.c[K:])
    _agree(streamed, plain, K)
    assert len(streamed) == K + N and streamed.pairs_searched()[1] == K * N + N * (N - 1) // 2
    got = _as(streamed.results())
    for v in (5, 128, 0, 64, K, K + 7, K + 100, K + 254, K + 255):               # what was planted is found, on both sides of K
        assert got[v] is not None and (got[v][0] is not None or got[v][1] is not None), v


# ---- 3. what add_streamed refuses -----------------------------------------------------------------------------------------------
def _refused(index, mt, cm, fhs, words, code=INVALID):
    before = _state(index)
    with pytest.raises(capi.NeedleError) as e:
        index.add_streamed(mt, cm, fhs)
    assert e.value.code == code and words in str(e.value), str(e.value)
    assert _state(index) == before, "a refused add_streamed leaves the index as it was"


def test_refusals_leave_the_index_as_it_was():
    rng = np.random.default_rng(83)
    corpus = Corpus(min_s=10)
    for (op,) in _planted(rng, 9, 300, _segments(rng, lengths=(100, 70, 60), bases=(7, 120, 200))):
        corpus.add_rows(op)
    low = [_min_len(10)]
    index, other, plain = (capi.Index(corpus.comparator()) for _ in range(3))
    for ix in (index, other, plain):
        ix.add(corpus.c[:3])
    new = corpus.c[3:5]
    rows = _lanes(new, 1)
    good_mt, good_cm = _season(index, new, low, 1)

    # origin: a matcher of another index, and one that no index made
    _refused(index, _season(other, new, low, 1)[0], good_cm, new, "not created from this index")
    loose = capi.Matcher.with_regions(_lanes(corpus.c[:3], 1), low * 3, 1, 2, 10)
    _feed_whole(loose, None, rows)
    _refused(index, loose, good_cm, new, "not created from this index")
    # incomplete, either object
    half = index.matcher(2)
    half.feed([rows[0], rows[1][:100]])
    half.finish([0])
    _refused(index, half, good_cm, new, "not complete")
    half_cm = capi.CrossMatcher.with_regions(2, [300], low, 10)
    half_cm.feed([rows[0], rows[1][:100]])
    half_cm.finish([0])
    _refused(index, good_mt, half_cm, new, "not complete")
    # lane counts and k, either object
    _refused(index, good_mt, good_cm, new[:1], "number of videos")
    _refused(index, good_mt, good_cm, new + [corpus.c[5]], "number of videos")
    three = corpus.c[3:6]
    _refused(index, _season(index, three, low, 1)[0], good_cm, three, "number of videos")
    _refused(index, good_mt, _season(index, three, low, 1)[1], new, "number of videos")
    two_regions = capi.CrossMatcher.with_regions(2, [300, 300], low * 2, 10)
    _feed_whole(two_regions, None, rows + rows)
    _refused(index, good_mt, two_regions, new, "number of videos")
    # a row against items_fed, and its hashes against either object's history (ONE word differs)
    _refused(index, good_mt, good_cm, [new[0], _copy_of(new[1], drop=1)], "not as long")
    for video, word in ((0, 0), (1, 299), (1, 150)):
        fhs = list(new)
        fhs[video] = _copy_of(new[video], flip=word)
        _refused(index, good_mt, good_cm, fhs, "hashes differ")
        other_rows = _lanes(fhs, 1)
        for feed_mt, feed_cm in ((other_rows, rows), (rows, other_rows)):        # only one of the two was fed something else
            mt, cm = index.matcher(2), capi.CrossMatcher.with_regions(2, [300], low, 10)
            _feed_whole(mt, None, feed_mt)
            _feed_whole(cm, None, feed_cm)
            _refused(index, mt, cm, new, "hashes differ")
    # the cross-matcher: a min_len that has lost runs, residents, none at all with two videos
    _refused(index, good_mt, _season(index, new, [low[0] + 1], 1)[1], new, "min_len")
    resident = index.crossmatcher(2, [300], low)
    _feed_whole(resident, None, rows)
    _refused(index, good_mt, resident, new, "resident")
    _refused(index, good_mt, None, new, "cross-matcher")
    # whatever add refuses, in the same words
    with pytest.raises(capi.NeedleError) as e:
        index.add_streamed(good_mt, good_cm, [])
    assert e.value.code == INVALID
    if capi.device_count() >= 2:                                                 # another device than the index's
        before = _state(index)
        capi.set_device(1)
        try:
            with pytest.raises(capi.NeedleError) as e:
                index.add_streamed(good_mt, good_cm, new)
            assert e.value.code == INVALID and "device" in str(e.value)
            with pytest.raises(capi.NeedleError) as e:
                index.matcher(2)
            assert e.value.code == INVALID and "device" in str(e.value)
        finally:
            capi.set_device(0)
        assert _state(index) == before
    # every one of them left the index and the good pair usable: a valid add_streamed equals the oracle and the plain index
    index.add_streamed(good_mt, good_cm, new)
    plain.add(new)
    _agree(index, plain, 3, corpus.expect(5))
    # ... and consumed: the index has changed since; so has it for a matcher made before an add, a remove or a replace
    _refused(index, good_mt, good_cm, new, "changed since")
    for change in (lambda ix: ix.add([corpus.c[5]]), lambda ix: ix.remove([0]), lambda ix: ix.replace([1], [corpus.c[6]])):
        stale = index.matcher(2)
        _feed_whole(stale, None, rows)
        change(index)
        _refused(index, stale, good_cm, new, "changed since")
    # after all that a fresh pair still works: 5 + 1 - 1 videos, video 1 replaced
    again = [corpus.c[7], corpus.c[0]]
    index.add_streamed(*_season(index, again, low, 1), again)
    view = Corpus(**corpus.cfg)
    view.c, view.o = [corpus.c[q] for q in (1, 6, 3, 4, 5, 7, 0)], [corpus.o[q] for q in (1, 6, 3, 4, 5, 7, 0)]
    assert _as(index.results()) == view.expect(7)


def test_refusals_in_the_words_of_add():
    """No ending data with endings on: refused as `add` refuses it, and the index goes on."""
    rng = np.random.default_rng(89)
    corpus = Corpus(endings=True, min_s=10)
    for op, en in _planted(rng, 4, 300, _segments(rng, lengths=(100, 70, 60), bases=(7, 120, 160)), endings=True):
        corpus.add_rows(op, en)
    index, plain = capi.Index(corpus.comparator()), capi.Index(corpus.comparator())
    for ix in (index, plain):
        ix.add(corpus.c[:2])
    new = corpus.c[2:]
    bare = [new[0], _copy_of(new[1], ending=False)]
    low = [_min_len(10)] * 2
    mt, cm = index.matcher(2), capi.CrossMatcher.with_regions(2, [300, 300], low, 10)
    _feed_whole(mt, cm, _lanes(bare, 2))
    _refused(index, mt, cm, bare, "no ending hash data", code=UNKNOWN)
    index.add_streamed(*_season(index, new, low, 2), new)
    plain.add(new)
    _agree(index, plain, 2, corpus.expect(4))
