"""-m gpu: the incremental index (needle_hip_index_*, csrc/index.cpp + the store in csrc/index_store.hip) against the oracle.
After every append the index's results must equal, to the nanosecond, oracle.run_with_frame_hashes over ALL videos added so
far in insertion order -- and capi.Comparator.run_with_frame_hashes over the same list -- while the scan saw only the new
pairs.  What can go wrong is ORDER (a video's candidates: its old pairs, then its pairs with the new videos), which videos'
results are recomputed, and what a failed append leaves behind."""
import os

import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests.test_gpu_parity import search_mode  # noqa: F401  (the fixture: every scan form)

pytestmark = pytest.mark.gpu
NS = O.NS
HD = O.duration_from_secs_f32(0.3)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _as(rs):
    return [None if r is None else (r.opening, r.ending) for r in rs]


class Corpus:
    """Videos as (capi.FrameHashes, oracle.FrameHashes) with the comparator settings of both sides."""

    def __init__(self, endings=False, threshold=10, min_s=10, padding=0.0):
        self.c, self.o = [], []
        self.cfg = dict(endings=endings, threshold=threshold, min_s=min_s, padding=padding)

    def add_rows(self, opening, ending=(), ts0=2_600_000_000, step=246_000_000, hd=HD):
        op = [(int(h), ts0 + i * step) for i, h in enumerate(opening)]
        en = [(int(h), ts0 + 7_000 * NS + i * step) for i, h in enumerate(ending)]
        self.c.append(capi.FrameHashes.new(op, en, hd))
        self.o.append(O.FrameHashes(op, en, hd))

    def add_capi(self, fh):
        h, t = fh.opening_data()
        eh, et = fh.ending_data()
        self.c.append(fh)
        self.o.append(O.FrameHashes(list(zip(h.tolist(), t.tolist())), list(zip(eh.tolist(), et.tolist())), fh.hash_duration()))

    def comparator(self):
        c = self.cfg
        return (capi.Comparator([f"v{k}.mkv" for k in range(max(2, len(self.c)))], include_endings=c["endings"],
                                hash_match_threshold=c["threshold"], min_opening_duration=c["min_s"],
                                min_ending_duration=c["min_s"], time_padding=c["padding"]))

    def oracle_comparator(self):
        c = self.cfg
        return O.Comparator(include_endings=c["endings"], hash_match_threshold=c["threshold"], min_opening_duration=c["min_s"] * NS,
                            min_ending_duration=c["min_s"] * NS, time_padding=O.duration_from_secs_f32(c["padding"]))

    def expect(self, n):
        want = _as(O.run_with_frame_hashes(self.oracle_comparator(), self.o[:n], threads=_threads()))
        full = self.comparator()
        full.videos = [f"v{k}.mkv" for k in range(max(2, n))]
        assert _as(full.run_with_frame_hashes(self.c[:n])) == want, "the full search disagrees with the oracle"
        return want


def _grow(corpus, index, steps, forms=None):
    """Appends in `steps` and checks every step: results == the full search, the scan saw exactly the new pairs.  forms:
    gets the scan form of every append (read before the full search launches scans of its own)."""
    n = len(index)
    for k in steps:
        index.add(corpus.c[n:n + k])
        if forms is not None:
            forms.append(capi.scan_last_launch()[0])
        n += k
        assert len(index) == n
        assert _as(index.results()) == corpus.expect(n), f"after growing to {n}"
        total, last = index.pairs_searched()
        assert last == n * (n - 1) // 2 - (n - k) * (n - k - 1) // 2
        assert total == n * (n - 1) // 2
    return index


def _planted(rng, n, kept, segments, endings=False, exact=False):
    """Random hash rows with shared segments planted (bit-identical with `exact`: equal simhashes, ties)."""
    out = []
    for v in range(n):
        regions = []
        for r in range(2 if endings else 1):
            h = rng.integers(0, 2 ** 32, kept, dtype=np.uint64).astype(np.uint32)
            for s, (seg, every, base) in enumerate(segments):
                a = base + 13 * (v % 5) + 31 * r
                if v % every or a + len(seg) >= kept:
                    continue
                flips = np.zeros(len(seg), np.uint32) if exact else \
                    (np.uint32(1) << rng.integers(0, 32, len(seg)).astype(np.uint32)) * (rng.random(len(seg)) < 0.5)
                h[a:a + len(seg)] = seg ^ flips
            regions.append(h)
        out.append(regions)
    return out


def _segments(rng, lengths=(110, 110, 95), every=(1, 2, 3), bases=(7, 260, 420)):
    return [(rng.integers(0, 2 ** 32, L, dtype=np.uint64).astype(np.uint32), e, b) for L, e, b in zip(lengths, every, bases)]


@pytest.mark.parametrize("endings", [False, True])
def test_tonal_library_grows_in_irregular_steps(endings):
    """synth.make_library, analyzed on the device; appends of 1, 1, 3, 7 and the rest, endings off and on."""
    n = 16
    eps = synth.make_library(n, 90.0, 20.0, 15.0 if endings else 0.0)
    paths = [f"/tmp/needle_index_ep{k}.wav" for k in range(n)]
    an = capi.Analyzer.from_files(paths).with_include_endings(endings)
    corpus = Corpus(endings=endings, min_s=10)
    for fh in an.run_pcm([e.pcm for e in eps], channels=1):
        corpus.add_capi(fh)
    index = _grow(corpus, capi.Index(corpus.comparator()), [1, 1, 3, 7, n - 12])
    res = index.results()
    assert all(r is not None and r.opening is not None for r in res), "the shared intro is found in every episode"


def test_planted_growth_with_endings_and_padding():
    rng = np.random.default_rng(5)
    corpus = Corpus(endings=True, min_s=15, padding=0.25)
    for op, en in _planted(rng, 14, 700, _segments(rng), endings=True):
        corpus.add_rows(op, en)
    _grow(corpus, capi.Index(corpus.comparator()), [2, 1, 4, 7])


def test_hostile_corpus_large_buckets_and_host_fallback(monkeypatch):
    """Silence against silence: buckets beyond a lane's 24 runs go to the large kernel; with that kernel switched off
    (NEEDLE_HIP_EPILOGUE_NO_LARGE, the switch the device epilogue's own tests use) the append's entries come from the
    host form.  Both equal the full search."""
    n, samples = 10, int(8 * 60 * 11025)
    gen = synth.DeviceLibrary(n, samples, 45.0, hostile=True)
    lib = capi.Library(n, opening_search_percentage=1.0)
    lib.set_pcm_device(gen.pointers(), [samples] * n)
    lib.analyze()
    corpus = Corpus(min_s=20)
    for v in range(n):
        corpus.add_capi(lib.frame_hashes(v))
    gen.free()
    _grow(corpus, capi.Index(corpus.comparator()), [3, 1, n - 4])
    before = capi.epilogue_host_fallbacks()
    monkeypatch.setenv("NEEDLE_HIP_EPILOGUE_NO_LARGE", "1")
    _grow(corpus, capi.Index(corpus.comparator()), [3, 1, n - 4])
    assert capi.epilogue_host_fallbacks() > before, "the appends with silent pairs fell back to the host entries"


def test_every_scan_form_on_appended_pairs(search_mode):
    rng = np.random.default_rng(11)
    corpus = Corpus(min_s=10)
    for (op,) in _planted(rng, 9, 900, _segments(rng)):
        corpus.add_rows(op)
    index = capi.Index(corpus.comparator())
    _grow(corpus, index, [4])
    forms = []
    _grow(corpus, index, [1, 4], forms)
    want = {"generic": 1, "band": 2, "sampled-mfma": 4}.get(search_mode, 3)
    assert forms == [want, want], (search_mode, forms)


def test_large_append_takes_the_matrix_pipe_by_itself(monkeypatch):
    """An append of 2528 new pairs (64 videos onto 8): the scan's matrix-pipe form is chosen automatically."""
    monkeypatch.delenv("NEEDLE_HIP_SCAN_MFMA", raising=False)
    rng = np.random.default_rng(3)
    corpus = Corpus(min_s=10)
    for (op,) in _planted(rng, 72, 640, _segments(rng, every=(1, 3, 7))):
        corpus.add_rows(op)
    index = capi.Index(corpus.comparator())
    forms = []
    _grow(corpus, index, [8, 64], forms)
    assert forms[1] == 4, forms


def test_ties_between_identical_episodes():
    """Bit-identical episodes: every candidate of a segment has the same score, the candidate index decides."""
    rng = np.random.default_rng(7)
    corpus = Corpus(min_s=10)
    base = rng.integers(0, 2 ** 32, 600, dtype=np.uint64).astype(np.uint32)
    for v in range(9):
        h = base.copy() if v % 3 else rng.integers(0, 2 ** 32, 600, dtype=np.uint64).astype(np.uint32)
        h[50:170] = base[50:170]
        corpus.add_rows(h)
    for (op,) in _planted(rng, 6, 600, _segments(rng), exact=True):
        corpus.add_rows(op)
    _grow(corpus, capi.Index(corpus.comparator()), [2, 1, 3, 1, 8])


def test_failed_appends_leave_the_index_as_it_was():
    rng = np.random.default_rng(13)
    corpus = Corpus(endings=True, min_s=15)
    rows = _planted(rng, 8, 600, _segments(rng), endings=True)
    for op, en in rows:
        corpus.add_rows(op, en)
    index = _grow(corpus, capi.Index(corpus.comparator()), [3])
    before = (len(index), _as(index.results()), index.pairs_searched())
    no_ending = capi.FrameHashes.new([(int(h), 2_600_000_000 + i * 246_000_000) for i, h in enumerate(rows[3][0])], [], HD)
    with pytest.raises(capi.NeedleError) as e:
        index.add([corpus.c[3], no_ending])
    assert "no ending hash data" in str(e.value)
    assert (len(index), _as(index.results()), index.pairs_searched()) == before
    _grow(corpus, index, [2, 3])

    # padding beyond a match's end: the reference panics on the subtraction
    rng = np.random.default_rng(17)
    pad = Corpus(min_s=10, padding=4000.0)
    for (op,) in _planted(rng, 5, 600, _segments(rng)):
        pad.add_rows(op)
    idx = capi.Index(pad.comparator())
    idx.add(pad.c[:1])
    before = (len(idx), _as(idx.results()), idx.pairs_searched())
    with pytest.raises(capi.NeedleError) as e:
        idx.add(pad.c[1:3])
    with pytest.raises(OverflowError):
        O.run_with_frame_hashes(pad.oracle_comparator(), pad.o[:3])
    assert (len(idx), _as(idx.results()), idx.pairs_searched()) == before
    # ... and a valid append after the failure still equals the full search
    ok = Corpus(min_s=10)
    ok.c, ok.o = [pad.c[0]], [pad.o[0]]
    rng = np.random.default_rng(19)
    for (op,) in _planted(rng, 3, 600, [(rng.integers(0, 2 ** 32, 20, dtype=np.uint64).astype(np.uint32), 1, 300)]):
        ok.add_rows(op)
    idx.add(ok.c[1:])
    assert _as(idx.results()) == _as(O.run_with_frame_hashes(pad.oracle_comparator(), ok.o))


def test_edge_cases_two_indexes_and_a_changed_comparator():
    rng = np.random.default_rng(23)
    corpus = Corpus(min_s=10)
    for (op,) in _planted(rng, 10, 600, _segments(rng)):
        corpus.add_rows(op)
    cmp = corpus.comparator()
    a, b = capi.Index(cmp), capi.Index(cmp)
    assert len(a) == 0 and a.results() == []
    a.add(corpus.c[:1])
    assert a.results() == [None] and a.pairs_searched() == (0, 0)
    # the comparator object changes after the indexes were made: neither index sees it
    cmp.with_min_opening_duration(60).with_hash_match_threshold(3).with_time_padding(1.0)
    cmp.handle()
    b.add(corpus.c[:3])
    a.add(corpus.c[1:4])
    b.add(corpus.c[3:7])
    a.add(corpus.c[4:10])
    b.add(corpus.c[7:10])
    want = corpus.expect(10)
    assert _as(a.results()) == want and _as(b.results()) == want
    assert a.pairs_searched()[0] == b.pairs_searched()[0] == 45


def test_results_buffer_too_short():
    rng = np.random.default_rng(29)
    corpus = Corpus(min_s=10)
    for (op,) in _planted(rng, 3, 300, _segments(rng, lengths=(60, 60, 60), bases=(7, 100, 200))):
        corpus.add_rows(op)
    index = capi.Index(corpus.comparator())
    index.add(corpus.c)
    res = (capi.CSearchResult * 3)()
    assert capi.lib().needle_hip_index_results(index._h, res, 2) == capi.ERROR_NAMES.index("InvalidArgument")
    assert capi.lib().needle_hip_index_results(index._h, res, 3) == 0
