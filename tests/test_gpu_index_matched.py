"""-m gpu: a streamed season into the index from its cross-matcher's runs (needle_hip_index_crossmatcher_new,
needle_hip_index_add_matched; csrc/index.cpp, the ingest in csrc/index_store.hip, the gather in csrc/crossmatch.hip).
The reference of every positive test is a second index that received the same videos through plain `add`, and the oracle
over the whole list: results, store sizes (the same entries in the same slots: the same run set after the filter) and
pairs_searched must agree while pairs_scanned says that nothing was scanned.  What can go wrong is the pair numbering (i-major
over K + N against the store's column-major ids), the runs the scan's problems exclude, which resident videos are
recomputed, and what a refused call leaves behind."""
import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests.test_gpu_index import Corpus, _as, _planted, _segments
from tests.test_gpu_library_rates import windows

pytestmark = pytest.mark.gpu
NS = O.NS
HD = O.duration_from_secs_f32(0.3)
STEP = 246_000_000                                                               # Corpus.add_rows' timestamps
INVALID, UNKNOWN = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("Unknown")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _min_len(min_s, step=STEP):
    """Comparator::min_run_length over evenly spaced timestamps: the fewest steps that span the minimum duration."""
    return -(-min_s * NS // step)


def _view(corpus, videos):
    """The corpus an index holds after edits: `videos` are positions of `corpus`, in the index's order."""
    v = Corpus(**corpus.cfg)
    v.c, v.o = [corpus.c[q] for q in videos], [corpus.o[q] for q in videos]
    return v


def _lanes(fhs, regions):
    """One hash array per lane: lane = video * regions + region."""
    out = []
    for fh in fhs:
        out.append(fh.opening_data()[0])
        if regions == 2:
            out.append(fh.ending_data()[0])
    return out


def _feed_ragged(m, rows, sizes=(1, 37, 64, 5)):
    """Feeds the lanes out of step: lane i takes the ragged sizes rotated by i, sits every fourth round out, then takes the
    rest in pieces of its own size, and is finished in the round its last item went in.  Lanes end in different rounds."""
    pos, step, rounds_of_finish = [0] * len(rows), 0, set()
    while not m.ready()[1]:
        chunk = []
        for i, x in enumerate(rows):
            take = 0 if (step + i) % 4 == 3 else sizes[(step + i) % len(sizes)] if step < 6 else 90 + 35 * i
            chunk.append(x[pos[i]: pos[i] + take] if take and pos[i] < len(x) else None)
            pos[i] = min(len(x), pos[i] + take)
        m.feed(chunk)
        ended = [i for i, x in enumerate(rows) if pos[i] == len(x) and not m.lane(i)[1]]
        if ended:
            m.finish(ended)
            rounds_of_finish.add(step)
        step += 1
    assert [m.lane(i) for i in range(len(rows))] == [(len(x), True) for x in rows]
    return len(rounds_of_finish)


def _season(index, fhs, min_len, regions=1, feed=_feed_ragged):
    """A complete matcher made from `index` that has been fed the videos `fhs`."""
    rows = _lanes(fhs, regions)
    max_items = [max(len(x) for x in rows[r::regions]) for r in range(regions)]
    m = index.crossmatcher(len(fhs), max_items, min_len)
    assert m.resident == len(index) and m.shape() == (len(fhs), regions)
    feed(m, rows)
    return m


def _state(index):
    """What a refused call must leave alone."""
    return len(index), _as(index.results()), index.pairs_searched(), index.pairs_scanned(), index.store_sizes()


def _agree(matched, plain, want, resident):
    """After an add_matched on `matched` and the add of the same videos on `plain`."""
    got = _as(matched.results())
    assert got == want, "add_matched disagrees with the oracle"
    assert got == _as(plain.results())
    assert matched.store_sizes() == plain.store_sizes()
    assert matched.pairs_searched() == plain.pairs_searched()
    assert matched.pairs_scanned()[1] == 0 and plain.pairs_scanned()[1] == plain.pairs_searched()[1]
    assert any(r is not None and r[0] is not None for r in got[:resident]) or resident == 0, "a resident video has an opening"
    assert any(r is not None and r[0] is not None for r in got[resident:]), "an arriving video has an opening"


def _plant(rows, seg, places, rng):
    """`seg` into rows[v][r] at `at` for (v, r, at) in places, with a flipped bit here and there (threshold 10)."""
    for v, r, at in places:
        flips = (np.uint32(1) << rng.integers(0, 32, len(seg)).astype(np.uint32)) * (rng.random(len(seg)) < 0.3)
        assert 0 <= at and at + len(seg) <= len(rows[v][r])
        rows[v][r][at:at + len(seg)] = seg ^ flips.astype(np.uint32)


def _library_and_season(endings, seed=41):
    """7 videos of 300 - 420 hashes, each of its own length: 4 known, 3 arriving.  Planted: the shared segments of
    test_gpu_index, one that ends on a resident row's last hash, one that ends on a lane's last item, one that starts at
    hash 0."""
    rng = np.random.default_rng(seed)
    regions = 2 if endings else 1
    lens = [[300, 333, 420, 371, 389, 312, 405], [310, 420, 345, 398, 301, 417, 366]]
    rows = _planted(rng, 7, 420, _segments(rng, lengths=(110, 80, 60), bases=(7, 150, 230)), endings=endings)
    rows = [[h[:lens[r][v]].copy() for r, h in enumerate(video)] for v, video in enumerate(rows)]
    new = lambda n: rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    for r in range(regions):
        n = lens[r]
        _plant(rows, new(70), [(1, r, n[1] - 70), (4, r, 100)], rng)             # ends on resident 1's last hash
        _plant(rows, new(90), [(2, r, 120), (5, r, n[5] - 90)], rng)             # ends on arriving 5's last item
        _plant(rows, new(64), [(0, r, 0), (6, r, 0), (3, r, 200)], rng)          # starts at hash 0 on both sides
    corpus = Corpus(endings=endings, min_s=10)
    for video in rows:
        corpus.add_rows(*video)
    return corpus, regions


# ---- 1. a season joins a library ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("endings", [False, True])
def test_a_season_joins_a_library(endings):
    corpus, regions = _library_and_season(endings)
    k, n = 4, 3
    matched, plain = capi.Index(corpus.comparator()), capi.Index(corpus.comparator())
    for ix in (matched, plain):
        ix.add(corpus.c[:3])
        ix.add(corpus.c[3:4])                                                    # two appends: arena offsets are not trivial
    rows = _lanes(corpus.c[k:], regions)
    assert any(len(x) < max(len(y) for y in rows[i % regions::regions]) for i, x in enumerate(rows)), "max_items exceeds some lanes"
    rounds = []
    m = _season(matched, corpus.c[k:], [_min_len(10)] * regions, regions, feed=lambda m, rows: rounds.append(_feed_ragged(m, rows)))
    assert rounds[0] >= 2, "the lanes finish in different rounds"
    assert m.ready()[0] >= 1
    before = matched.pairs_scanned()
    matched.add_matched(m, corpus.c[k:])
    plain.add(corpus.c[k:])
    assert len(matched) == k + n
    _agree(matched, plain, corpus.expect(k + n), k)
    assert matched.pairs_scanned() == (before[0], 0)
    assert matched.pairs_searched()[1] == k * n + n * (n - 1) // 2


# ---- 2. a fresh season into an empty index -----------------------------------------------------------------------------------
def test_a_fresh_season_into_an_empty_index():
    corpus, _ = _library_and_season(False, seed=43)
    matched, plain = capi.Index(corpus.comparator()), capi.Index(corpus.comparator())
    fhs = corpus.c[:4]
    m = _season(matched, fhs, [_min_len(10)])
    assert m.resident == 0 and m.ready()[0] >= 1
    matched.add_matched(m, fhs)
    plain.add(fhs)
    _agree(matched, plain, corpus.expect(4), 0)
    assert matched.pairs_scanned() == (0, 0) and matched.pairs_searched() == (6, 6)


# ---- 3. two seasons in a row, then edits -------------------------------------------------------------------------------------
def test_two_seasons_in_a_row_then_edits():
    rng = np.random.default_rng(47)
    corpus = Corpus(min_s=10)
    for (op,) in _planted(rng, 11, 320, _segments(rng, lengths=(100, 70, 60), bases=(7, 120, 200))):
        corpus.add_rows(op)
    matched, plain = capi.Index(corpus.comparator()), capi.Index(corpus.comparator())
    for ix in (matched, plain):
        ix.add(corpus.c[:3])
    held = [0, 1, 2]

    def season(videos):
        fhs = [corpus.c[q] for q in videos]
        resident = len(matched)
        m = _season(matched, fhs, [_min_len(10)])
        assert m.ready()[0] >= 1
        matched.add_matched(m, fhs)
        plain.add(fhs)
        held.extend(videos)
        _agree(matched, plain, _view(corpus, held).expect(len(held)), resident)

    def edited():
        assert _as(matched.results()) == _as(plain.results()) == _view(corpus, held).expect(len(held))
        assert matched.store_sizes() == plain.store_sizes()

    season([3, 4])
    season([5, 6])                                                               # a matcher from the grown index
    for ix in (matched, plain):
        ix.remove([1, 4])                                                        # one old, one streamed
    del held[4], held[1]
    edited()
    season([7, 8])                                                               # a matcher from the rebuilt store
    for ix in (matched, plain):
        ix.replace([2], [corpus.c[9]])
    held[2] = 9
    edited()
    for ix in (matched, plain):
        ix.add([corpus.c[10]])
    held.append(10)
    edited()
    assert matched.pairs_searched() == plain.pairs_searched()
    assert matched.pairs_scanned()[0] < plain.pairs_scanned()[0] == plain.pairs_searched()[0]


# ---- 4. the per-pair bound ---------------------------------------------------------------------------------------------------
def test_the_per_pair_bound_drops_what_the_scan_would_not_report():
    """Rows with timestamps 123 ms apart need runs twice as long as rows 246 ms apart; the matcher had the smaller bound for
    every pair.  A segment between the two bounds, in a pair that needs the larger one, is in the matcher's list and must not
    reach the store."""
    rng = np.random.default_rng(53)
    fine, coarse = STEP // 2, STEP
    low, high = _min_len(10, coarse), _min_len(10, fine)
    assert (low, high) == (41, 82)
    steps = [coarse, fine, coarse, fine, coarse]                                 # 2 known, 3 arriving
    new = lambda n: rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    rows = [[new(400)] for _ in steps]
    between = (low + high) // 2
    assert low < between < high
    _plant(rows, new(between), [(1, 0, 30), (2, 0, 200)], rng)                   # (fine, coarse): needs `high`
    _plant(rows, new(between), [(3, 0, 250), (4, 0, 40)], rng)                   # (fine, coarse) among the arriving
    _plant(rows, new(high + 20), [(1, 0, 150), (3, 0, 60)], rng)                 # long enough for any pair
    _plant(rows, new(low + 10), [(0, 0, 300), (2, 0, 20), (4, 0, 310)], rng)     # coarse pairs: the small bound is theirs
    corpus = Corpus(min_s=10)
    for (op,), step in zip(rows, steps):
        corpus.add_rows(op, step=step)
    matched, plain = capi.Index(corpus.comparator()), capi.Index(corpus.comparator())
    for ix in (matched, plain):
        ix.add(corpus.c[:2])
    assert matched.store_sizes()[1] == 0                                         # the two known videos share nothing
    m = _season(matched, corpus.c[2:], [low])
    matched.add_matched(m, corpus.c[2:])
    plain.add(corpus.c[2:])
    assert m.ready()[0] > matched.store_sizes()[1] >= 1, "the filter dropped runs the matcher reported"
    lens = sorted(int(x) for x in m.runs()["len"])
    assert any(low <= x < high for x in lens)
    _agree(matched, plain, corpus.expect(5), 2)


# ---- 5. crowded buckets ------------------------------------------------------------------------------------------------------
def _crowded():
    rng = np.random.default_rng(59)
    new = lambda n: rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    rows = [[new(220)] for _ in range(4)]
    rows[1][0][60:108] = rows[3][0][100:148] = np.uint32(0x9E3779B9)             # 48 identical hashes on both sides
    _plant(rows, new(40), [(0, 0, 10), (2, 0, 150)], rng)
    corpus = Corpus(min_s=5)
    for (op,) in rows:
        corpus.add_rows(op)
    return corpus


@pytest.mark.parametrize("no_large", [False, True])
def test_crowded_buckets_large_kernel_and_host_fallback(no_large, monkeypatch):
    corpus = _crowded()
    min_len = _min_len(5)
    assert 18 <= min_len <= 22
    matched, plain = capi.Index(corpus.comparator()), capi.Index(corpus.comparator())
    for ix in (matched, plain):
        ix.add(corpus.c[:2])
    m = _season(matched, corpus.c[2:], [min_len])
    runs = m.runs()
    crowded = max(np.bincount(runs["problem"].astype(np.int64)))
    assert crowded > 24, "one bucket holds more runs than a lane orders (kEpilogueBucketLimit)"
    if no_large:
        monkeypatch.setenv("NEEDLE_HIP_EPILOGUE_NO_LARGE", "1")
    before = capi.epilogue_host_fallbacks()
    matched.add_matched(m, corpus.c[2:])
    fell_back = capi.epilogue_host_fallbacks() - before
    assert fell_back == (1 if no_large else 0), "the ingested list goes through the host entries when the large kernel is off"
    plain.add(corpus.c[2:])
    _agree(matched, plain, corpus.expect(4), 2)


# ---- 6. from PCM -------------------------------------------------------------------------------------------------------------
def test_from_pcm_through_feeder_and_matcher_into_the_index():
    eps = synth.make_library(5, 90.0, 20.0, 0.0)
    names = [f"/tmp/needle_matched_ep{k}.wav" for k in range(5)]
    full = capi.Analyzer.from_files(names).run_pcm([e.pcm for e in eps], channels=1)
    cmp = capi.Comparator(names, min_opening_duration=10)
    want = _as(cmp.run_with_frame_hashes(full))
    assert all(r is not None and r[0] is not None for r in want)
    index = capi.Index(cmp)
    index.add(full[:2])
    opening = [e.pcm[: windows(len(e.pcm), 1, 11025, endings=False)[0][1]] for e in eps[2:]]   # what the analyzer fingerprints
    longest = max(capi.feeder_num_ready(len(x), 11025, 1, 2, True) for x in opening)
    f = capi.Feeder(3, 1, 11025, capi.SAMPLE_S16, 2)
    m = index.crossmatcher(3, [longest], [30])
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
    for got, ref in zip(streamed, full[2:]):
        assert got.opening_data()[0].tolist() == ref.opening_data()[0].tolist()
    index.add_matched(m, streamed)
    assert _as(index.results()) == want
    assert index.pairs_scanned() == (1, 0) and index.pairs_searched() == (10, 9)


# ---- 7. what add_matched refuses ---------------------------------------------------------------------------------------------
def _refused(index, matcher, fhs, words, code=INVALID):
    before = _state(index)
    with pytest.raises(capi.NeedleError) as e:
        index.add_matched(matcher, fhs)
    assert e.value.code == code and words in str(e.value), str(e.value)
    assert _state(index) == before, "a refused add_matched leaves the index as it was"


def _copy_of(fh, drop=0, flip=None, ending=True):
    """The video again, less its last `drop` opening hashes, with one bit of hash `flip` flipped, or without its ending."""
    h, ts = fh.opening_data()
    eh, ets = fh.ending_data()
    h = h.copy()
    if flip is not None:
        h[flip] ^= np.uint32(1 << 17)
    n = len(h) - drop
    return capi.FrameHashes.new(list(zip(h[:n].tolist(), ts[:n].tolist())), list(zip(eh.tolist(), ets.tolist())) if ending else [],
                                fh.hash_duration())


def test_refusals_leave_the_index_as_it_was():
    rng = np.random.default_rng(61)
    corpus = Corpus(min_s=10)
    for (op,) in _planted(rng, 8, 300, _segments(rng, lengths=(100, 70, 60), bases=(7, 120, 200))):
        corpus.add_rows(op)
    low = _min_len(10)
    index, other, plain = (capi.Index(corpus.comparator()) for _ in range(3))
    for ix in (index, other, plain):
        ix.add(corpus.c[:3])
    new = corpus.c[3:5]
    rows = _lanes(new, 1)
    cap = [max(len(x) for x in rows)]

    _refused(index, _season(other, new, [low]), new, "not created from this index")
    loose = capi.CrossMatcher.with_resident(_lanes(corpus.c[:3], 1), 2, cap, [low], 10)
    _feed_ragged(loose, rows)
    _refused(index, loose, new, "not created from this index")
    half = index.crossmatcher(2, cap, [low])
    half.feed([rows[0], rows[1][:100]])
    half.finish([0])
    _refused(index, half, new, "not complete")
    good = _season(index, new, [low])
    _refused(index, good, new[:1], "number of videos")
    _refused(index, good, new + [corpus.c[5]], "number of videos")
    _refused(index, good, [new[0], _copy_of(new[1], drop=1)], "not as long")
    for video, word in ((0, 0), (1, 299), (1, 150)):                             # ONE hash word differs
        fhs = list(new)
        fhs[video] = _copy_of(new[video], flip=word)
        _refused(index, good, fhs, "hashes differ")
    _refused(index, _season(index, new, [low + 1]), new, "min_len")
    # every one of them left `good` usable: a valid add_matched equals the oracle and the plain index
    index.add_matched(good, new)
    plain.add(new)
    _agree(index, plain, corpus.expect(5), 3)
    # ... and consumed: the index has changed since; so has it for a matcher made before an add, a remove or a replace
    _refused(index, good, new, "changed since")
    for change in (lambda ix: ix.add([corpus.c[5]]), lambda ix: ix.remove([0]), lambda ix: ix.replace([1], [corpus.c[6]])):
        stale = index.crossmatcher(2, cap, [low])
        change(index)
        _refused(index, stale, new, "changed since")
    with pytest.raises(capi.NeedleError) as e:
        index.add_matched(good, [])
    assert e.value.code == INVALID
    # after all that a fresh matcher still works: 5 + 1 - 1 videos, video 1 replaced
    held = [1, 6, 3, 4, 5]
    again = [corpus.c[7], corpus.c[0]]
    index.add_matched(_season(index, again, [low]), again)
    assert _as(index.results()) == _view(corpus, held + [7, 0]).expect(7)


def test_refusals_in_the_words_of_add():
    """No ending data with endings on; padding beyond a match's end (the reference panics on the subtraction)."""
    rng = np.random.default_rng(67)
    corpus = Corpus(endings=True, min_s=10)
    for op, en in _planted(rng, 4, 300, _segments(rng, lengths=(100, 70, 60), bases=(7, 120, 160)), endings=True):
        corpus.add_rows(op, en)
    index, plain = capi.Index(corpus.comparator()), capi.Index(corpus.comparator())
    for ix in (index, plain):
        ix.add(corpus.c[:2])
    new = corpus.c[2:]
    bare = [new[0], _copy_of(new[1], ending=False)]
    m = index.crossmatcher(2, [300, 300], [_min_len(10)] * 2)
    rows = _lanes(bare, 2)
    m.feed(rows)
    m.finish()
    _refused(index, m, bare, "no ending hash data", code=UNKNOWN)
    before = _state(plain)
    with pytest.raises(capi.NeedleError) as e:
        plain.add(bare)
    assert "no ending hash data" in str(e.value) and _state(plain) == before
    good = _season(index, new, [_min_len(10)] * 2, regions=2)
    index.add_matched(good, new)
    plain.add(new)
    _agree(index, plain, corpus.expect(4), 2)

    rng = np.random.default_rng(17)
    pad = Corpus(min_s=10, padding=4000.0)
    for (op,) in _planted(rng, 5, 600, _segments(rng)):
        pad.add_rows(op)
    idx = capi.Index(pad.comparator())
    idx.add(pad.c[:1])
    m = _season(idx, pad.c[1:3], [_min_len(10)])
    assert m.ready()[0] >= 1
    _refused(idx, m, pad.c[1:3], "overflow when subtracting", code=UNKNOWN)
    with pytest.raises(OverflowError):
        O.run_with_frame_hashes(pad.oracle_comparator(), pad.o[:3])


def test_another_device_is_refused():
    if capi.device_count() < 2:
        pytest.skip(f"needs 2 GPUs, this box has {capi.device_count()}")
    rng = np.random.default_rng(71)
    corpus = Corpus(min_s=10)
    for (op,) in _planted(rng, 4, 300, _segments(rng, lengths=(100, 70, 60), bases=(7, 120, 200))):
        corpus.add_rows(op)
    index = capi.Index(corpus.comparator())
    index.add(corpus.c[:2])
    m = _season(index, corpus.c[2:], [_min_len(10)])
    before = _state(index)
    capi.set_device(1)
    try:
        with pytest.raises(capi.NeedleError) as e:
            index.add_matched(m, corpus.c[2:])
        assert e.value.code == INVALID and "device" in str(e.value)
        with pytest.raises(capi.NeedleError) as e:
            index.crossmatcher(2, [300], [_min_len(10)])
        assert e.value.code == INVALID and "device" in str(e.value)
    finally:
        capi.set_device(0)
    assert _state(index) == before
    index.add_matched(m, corpus.c[2:])
    assert _as(index.results()) == corpus.expect(4)
