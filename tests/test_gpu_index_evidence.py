"""-m gpu: match evidence of the incremental index (needle_hip_index_evidence: best_match_kernel under its third video policy
and match_evidence_kernel, csrc/epilogue_kernels.h, csrc/index_store.hip) against the host definition
(needle_hip_comparator_results_from_runs_evidence over the same videos and the ORACLE's run list; tests/test_evidence_cpu.py
checks that one against a model).  What can go wrong on the device: the slot behind a winner's candidate index (prefix sums
over more than 256 pair slots, openings before endings inside a slot), the role (source or destination), partners counted per
slot, positions after edits, and anything the call might leave behind."""
import os

import numpy as np
import pytest

from needle_amd import capi
from oracle import oracle as O
from tests import best_match_model as M
from tests.test_gpu_feeder_formats import timed
from tests.test_gpu_index import Corpus, _as, _planted, _segments
from tests.test_gpu_index_matched import _library_and_season, _min_len, _plant, _season

pytestmark = pytest.mark.gpu
NS = O.NS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _rows(fhs, endings):
    return [[fh.opening_data()[0]] + ([fh.ending_data()[0]] if endings else []) for fh in fhs]


def _host(corpus, fhs):
    """(results, evidence, oracle runs) of the host definition over `fhs`, the runs from the oracle's scan."""
    cfg = corpus.cfg
    runs = M.oracle_runs(_rows(fhs, cfg["endings"]), cfg["threshold"], M.min_len_for(cfg["min_s"]), threads=_threads())
    cmp = corpus.comparator()
    cmp.videos = [f"v{k}.mkv" for k in range(max(2, len(fhs)))]
    results, evidence = cmp.results_from_runs_evidence(fhs, runs)
    return results, evidence, runs


def _same(got, want):
    assert len(got) == len(want)
    for v, (g, w) in enumerate(zip(got, want)):
        for name in ("opening", "ending"):
            assert M.same_evidence(getattr(g, name), getattr(w, name)), (v, name, getattr(g, name), getattr(w, name))


def _consistent(index, evidence, corpus, fhs):
    """The two equations of needle_hip.h against index.results()."""
    pad = O.duration_from_secs_f32(corpus.cfg["padding"])
    for v, (res, ev) in enumerate(zip(index.results(), evidence)):
        for name in ("opening", "ending"):
            e, r = getattr(ev, name), None if res is None else getattr(res, name)
            assert (e is None) == (r is None), (v, name)
            if e is not None:
                assert r == (e.interval[0] + pad, e.interval[1] - pad - fhs[v].hash_duration()), (v, name)


def _check(index, corpus, fhs):
    """index.evidence() == the host definition over the index's current list; both consistent with index.results()."""
    results, want, runs = _host(corpus, fhs)
    assert _as(index.results()) == _as(results)
    got = index.evidence()
    _same(got, want)
    _consistent(index, got, corpus, fhs)
    return got, runs


def _corpus(rows, **cfg):
    corpus = Corpus(**cfg)
    for video in rows:
        corpus.add_rows(*video)
    return corpus


# ---- 1. the small planted library ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("endings,padding,seed", [(False, 0.0, 101), (True, 0.25, 102)])
def test_small_planted_library(endings, padding, seed):
    corpus = _corpus(M.planted_library(seed, endings), endings=endings, min_s=10, padding=padding)
    index = capi.Index(corpus.comparator())
    assert index.evidence() == []
    index.add(corpus.c[:1])
    assert index.evidence() == [capi.SearchEvidence(None, None)]               # one video: no pair
    index.add(corpus.c[1:4])
    index.add(corpus.c[4:])
    got, _ = _check(index, corpus, corpus.c)
    assert all(e.opening is not None for e in got) and got[3].opening.partner in (4, 5)
    assert all(e.ending is None for e in got) if not endings else got[5].ending is not None and got[0].ending is None
    ev = (capi.CSearchEvidence * 6)()
    assert capi.lib().needle_hip_index_evidence(index._h, ev, 5) == capi.ERROR_NAMES.index("InvalidArgument")
    assert capi.lib().needle_hip_index_evidence(index._h, None, 6) == capi.ERROR_NAMES.index("NullArgument")
    assert capi.lib().needle_hip_index_evidence(index._h, ev, 6) == 0


# ---- 2. slot and stage boundaries ---------------------------------------------------------------------------------------------
def test_more_than_256_pair_slots_and_512_candidates():
    """260 videos of 200 hashes that all share one 80-hash segment in both regions: 259 pair slots per video (the kernels walk
    them 256 at a time: two rounds, the second of 3), up to 518 candidates per video (beyond best_match's 512)."""
    rng = np.random.default_rng(211)
    n, kept = 260, 200
    new = lambda k: rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
    rows = [[new(kept), new(kept)] for _ in range(n)]
    late = (5, 257, 258, 259)                                                  # these share 12 hashes more: video 5's winner is
    for r in range(2):                                                         # behind its 256th slot, candidate 512 or later
        seg = new(92)
        _plant(rows, seg[:80], [(v, r, 15 + 7 * ((v + 3 * r) % 13)) for v in range(n) if v not in late], rng)
        _plant(rows, seg, [(v, r, 15 + 7 * ((v + 3 * r) % 13)) for v in late], rng)
    corpus = _corpus(rows, endings=True, min_s=15)                             # 61 hashes: the 80-hash plant qualifies
    assert 61 == M.min_len_for(15) < 80 < M.min_len_for(20)
    index = capi.Index(corpus.comparator())
    index.add(corpus.c[:200])
    index.add(corpus.c[200:])
    got, _ = _check(index, corpus, corpus.c)
    assert max(e.opening.candidates for e in got) > 512
    for e in (got[5].opening, got[5].ending):
        assert e.partner in late and e.candidate >= 512, "a winner behind the 256th slot"


# ---- 3. crowded buckets ---------------------------------------------------------------------------------------------------------
def test_crowded_buckets_large_kernel_and_host_entries(monkeypatch):
    """Stretches of one repeated hash in three videos: every diagonal of a 48 x 48 block is a run, so their pairs' buckets
    hold more runs than a lane orders.  One append takes the host-entries fallback, the next the large kernel; the evidence
    is the host definition's either way, and the run it names is one the oracle found."""
    rng = np.random.default_rng(59)
    new = lambda k: rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
    rows = [[new(220)] for _ in range(6)]
    rows[1][0][60:108] = rows[3][0][100:148] = rows[4][0][20:68] = np.uint32(0x9E3779B9)
    _plant(rows, new(40), [(0, 0, 10), (2, 0, 150), (5, 0, 90)], rng)
    corpus = _corpus(rows, min_s=5)
    index = capi.Index(corpus.comparator())
    index.add(corpus.c[:2])
    before = capi.epilogue_host_fallbacks()
    monkeypatch.setenv("NEEDLE_HIP_EPILOGUE_NO_LARGE", "1")
    index.add(corpus.c[2:4])
    assert capi.epilogue_host_fallbacks() == before + 1, "this append's entries came from the host"
    monkeypatch.delenv("NEEDLE_HIP_EPILOGUE_NO_LARGE")
    index.add(corpus.c[4:])
    assert capi.epilogue_host_fallbacks() == before + 1
    got, runs = _check(index, corpus, corpus.c)
    assert np.bincount(runs["problem"].astype(np.int64)).max() > 24, "a bucket beyond kEpilogueBucketLimit"
    assert got[1].opening.candidates > 48 and got[1].opening.partners == 2 and got[1].opening.partner in (3, 4)
    pairs = [(i, j) for i in range(6) for j in range(i + 1, 6)]
    ts = M.timestamps(rows)
    named = 0
    for v, e in enumerate(got):
        e = e.opening
        i, j = (v, e.partner) if e.is_source else (e.partner, v)
        assert i < j
        src, dst = (e.interval, e.partner_interval) if e.is_source else (e.partner_interval, e.interval)
        src_hash, dst_hash = (e.match_hash, e.partner_hash) if e.is_source else (e.partner_hash, e.match_hash)
        mine = runs[runs["problem"] == pairs.index((i, j))]                     # one region: problem = pair
        assert any((ts[i][0][r["src_end"] - r["len"]], ts[i][0][r["src_end"]]) == src and
                   (ts[j][0][r["dst_end"] - r["len"]], ts[j][0][r["dst_end"]]) == dst and
                   (r["src_match_hash"], r["dst_match_hash"]) == (src_hash, dst_hash) for r in mine), (v, e)
        named += 1
    assert named == 6


# ---- 4. edits -------------------------------------------------------------------------------------------------------------------
def test_after_remove_and_replace_partners_are_current_positions():
    rng = np.random.default_rng(61)
    rows = _planted(rng, 10, 420, _segments(rng, lengths=(110, 80, 60), bases=(7, 150, 260)), endings=True)
    corpus = _corpus(rows, endings=True, min_s=10)
    index = capi.Index(corpus.comparator())
    index.add(corpus.c[:9])
    held = list(range(9))

    def fresh_agrees():
        fhs = [corpus.c[q] for q in held]
        fresh = capi.Index(corpus.comparator())
        fresh.add(fhs)
        got, _ = _check(index, corpus, fhs)
        assert got == fresh.evidence()
        assert all(e.opening is None or e.opening.partner < len(held) for e in got)
        return got

    before = fresh_agrees()
    index.remove([0, 3])
    del held[3], held[0]
    after = fresh_agrees()
    assert any(b.opening and b.opening.partner in (0, 3) for b in before[1:3] + before[4:]), "a winner's partner was removed"
    assert len(after) == 7
    index.replace([2], [corpus.c[9]])
    held[2] = 9
    fresh_agrees()


# ---- 5. a streamed season -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("endings", [False, True])
def test_streamed_season_equals_the_twin_built_by_add(endings):
    corpus, regions = _library_and_season(endings)
    matched, plain = capi.Index(corpus.comparator()), capi.Index(corpus.comparator())
    for ix in (matched, plain):
        ix.add(corpus.c[:4])
    m = _season(matched, corpus.c[4:], [_min_len(10)] * regions, regions)
    matched.add_matched(m, corpus.c[4:])
    plain.add(corpus.c[4:])
    got = matched.evidence()
    assert got == plain.evidence()
    assert any(e.opening is not None and e.opening.partner >= 4 for e in got[:4]), "a resident video's winner is an arriving one"
    _consistent(matched, got, corpus, corpus.c)


# ---- 6. read-only ---------------------------------------------------------------------------------------------------------------
def test_evidence_changes_nothing():
    rng = np.random.default_rng(67)
    rows = _planted(rng, 9, 420, _segments(rng, lengths=(110, 80, 60), bases=(7, 150, 260)))
    corpus = _corpus(rows, min_s=10)
    asked, twin = capi.Index(corpus.comparator()), capi.Index(corpus.comparator())
    for ix in (asked, twin):
        ix.add(corpus.c[:3])
        ix.add(corpus.c[3:6])
    state = lambda ix: (len(ix), _as(ix.results()), ix.store_sizes(), ix.pairs_searched(), ix.pairs_scanned())
    before = state(asked)
    first = asked.evidence()
    assert state(asked) == before == state(twin)
    assert asked.evidence() == first, "nothing is kept: the second call computes the same"
    launches = [timed(lambda ix=ix: ix.add(corpus.c[6:])) for ix in (asked, twin)]
    assert launches[0] == launches[1] and launches[0].get("index_best_match") == 1 and "index_evidence" not in launches[0]
    assert state(asked) == state(twin)
    assert _as(asked.results()) == corpus.expect(9)
    assert asked.evidence() == twin.evidence()
    shown = timed(lambda: asked.evidence())
    assert shown == {"index_evidence_match": 1, "index_evidence": 1}, "two launches, one wait"
