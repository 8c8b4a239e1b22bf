"""-m gpu: the link counts of best_match_kernel (csrc/epilogue_kernels.h) at the bound's edge and at every size at which the
kernel takes another path.  links[k] = #{b : popcount(h_k ^ h_b) < bound}, bound = t + t / 2 (comparator.rs:434-454), and both
of the kernel's paths encode the bound in arithmetic: the matrix path presets its accumulators to 32 - 2 bound and reads sign
bits, sixteen to a word, two tiles to a popcount, 512 candidates to a stage, and takes the zero rows of the last block out
again once bound > 16; the dedup path (from 512 candidates, up to 1536 distinct hashes) sums multiplicities over a 2048-slot
table whose probes wrap.  The libraries are the hubs and spokes of tests/link_tables.py, whose candidate hashes are chosen one
by one (tests/test_link_tables_cpu.py proves them against the oracle): all of a hub's candidates last equally long, so the
links alone pick its winner, and evidence shows the winner's index and support.  Every case builds an Index in two uneven
appends; results against the oracle's full search, evidence field for field against tests/best_match_model.py, the hub's
support against the O(c^2) count over the targets alone, and no host fallback.

The three lists of 1536 and 1537 candidates come from 768 and 769 spokes that hold one segment in EACH region (one run per
(pair, region) bucket all the same, the hub's candidates in target order), not from one spoke per candidate: at 1538 videos
the reference's own per-video pass over all pairs takes 13 s a library, measured on rows of three hashes -- the
length of the segments, which a smaller minimum duration would shorten, is not what costs.

Wall time of every test on one MI355X (pytest --durations, seconds; the whole module 11.7, tests/test_gpu_index_evidence.py on
the same machine 1.7 for its eight tests, 0.58 its longest): the bound's edge 0.29 (t = 1, the first to touch the device),
0.07 - 0.12 (the others), t = 0 0.04; block edges 0.10 - 0.12 (1 .. 65 candidates), 0.29 - 0.34 (511); the dedup path at 512 and
513 candidates 0.43 - 0.51; the limit cases 1.11 - 1.18 (t = 10), 1.29 - 1.32 (t = 12); slots 0.02; the other policies 0.01 - 0.08,
on the dedup path 0.17.

Sabotage (scratch builds, one line of best_match_kernel each, none committed): which of these tests fail.
  32 - 2 bound -> 30 - 2 bound: 21 tests -- every bound's-edge case and t = 0, all block edges, all limit cases, slots, and of
    the other policies edge-t11 and both block cases.
  `if (preset < 0) cnt -= pad` removed: the bound's edge at t = 12 and 14, block edges at t = 12 (both), the dedup path at t = 12
    (its spokes' lists of one candidate), the limit cases at t = 12 (all three).
  `b0 == 0 ? 0u : links[k]` -> `0u`: the limit cases of 1537 distinct hashes, t = 10 and 12 (the only lists of several stages).
  `< pr.bound` -> `<= pr.bound` in the dedup sum: the dedup path at 512 and 513 (t = 10, 12) and the limit cases of 1536
    distinct hashes (1536 and 1537 candidates, t = 10, 12).
  kMaxDistinct 1536 -> 1535: NO test fails, and none can by results: a list of 1536 distinct hashes then takes the matrix
    path, which counts the same links; nothing the library shows says which path ran.
  `(sl + 1) & (kSlots - 1)` -> `sl + 1` reads beyond the table and is not run: tests/test_link_tables_cpu.py shows on the table
    model that the collide palettes' probes reach slots 0 .. 4 (2048 .. 2052 without the wrap).
"""
import os

import numpy as np
import pytest

from needle_amd import capi
from oracle import oracle as O
from tests import best_match_model as M
from tests import link_tables as T
from tests.test_gpu_index import Corpus, _as

pytestmark = pytest.mark.gpu
NS = O.NS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _corpus(case, copies=1):
    """The case's videos, each `copies` times in a row (two shows with interleaved labels)."""
    corpus = Corpus(endings=case.endings, threshold=case.t, min_s=case.min_s)
    for video in case.rows():
        for _ in range(copies):
            corpus.add_rows(*video)
    return corpus


def _oracle(corpus, fhs=None):
    return _as(O.run_with_frame_hashes(corpus.oracle_comparator(), corpus.o if fhs is None else fhs, threads=_threads()))


def _index(corpus):
    index = capi.Index(corpus.comparator())
    first = len(corpus.c) // 3 + 1
    index.add(corpus.c[:first])
    index.add(corpus.c[first:])
    return index


def _hub_support(case, got):
    """The hub's winners are the ones the targets alone name, with the support the O(c^2) count gives."""
    for h, table in enumerate(case.tables):
        want = case.winners(h)
        count = T.links(table, case.bound)
        for which, name in enumerate(("opening", "ending")):
            e = getattr(got[h], name)
            if want[which] is None:
                assert e is None, (case, h, name, e)
                continue
            assert e is not None, (case, h, name, want[which])
            assert (e.candidate, e.support) == want[which] and e.support == count[e.candidate], (case, h, name, e, want[which])
            assert e.candidates == len(table) and e.partner == case.spoke_of(h, e.candidate) and e.is_source
            assert e.match_hash == int(table[e.candidate])


def _check(case):
    """Index results == the oracle, index evidence == the model, the hub's support == links(targets), no host fallback."""
    before = capi.epilogue_host_fallbacks()
    corpus = _corpus(case)
    index = _index(corpus)
    assert _as(index.results()) == _oracle(corpus), case
    rows = case.rows()
    runs = M.oracle_runs(rows, case.t, case.min_len, threads=_threads())
    min_ns = (case.min_s * NS, case.min_s * NS)
    _, want = M.evidence_model(M.timestamps(rows), runs, case.t, min_ns, case.endings)
    got = index.evidence()
    assert len(got) == len(want)
    for v, (g, w) in enumerate(zip(got, want)):
        for which, name in enumerate(("opening", "ending")):
            assert M.same_evidence(getattr(g, name), w[which]), (case, v, name, getattr(g, name), w[which])
    _hub_support(case, got)
    assert capi.epilogue_host_fallbacks() == before, "the device epilogue took every append"
    return got


# ---- (a) the bound's edge -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 10, 11, 12, 14])
def test_the_bounds_edge_at_every_rotation(t):
    """Bounds 1, 3, 15, 16 (preset 0), 18 (the first with the pad correction) and 21: two centres A and ~A with satellites at
    exactly bound - 1 and bound, sixteen hubs that hold the table at its sixteen rotations.  (winner, support) under bound - 1,
    bound and bound + 1 are pairwise different at every rotation (test_link_tables_cpu.py)."""
    got = _check(T.edge_case(t))
    assert all(e.opening is not None for e in got[:16])


def test_threshold_zero_nobody_links():
    """bound = 0: no candidate links, not even to itself; every video with candidates has a result with neither side."""
    case = T.edge_case(0)
    corpus = _corpus(case)
    index = _index(corpus)
    res = index.results()
    assert _as(res) == _oracle(corpus) == [(None, None)] * len(corpus.c)
    assert index.evidence() == [capi.SearchEvidence(None, None)] * len(corpus.c)


# ---- (b) block and stage edges of the matrix path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", T.BLOCK_SIZES, ids=["c1-65", "c511"])
@pytest.mark.parametrize("t", [10, 12])
def test_block_edges_of_the_matrix_path(t, sizes):
    """Hubs of 1, 2, 31, 32, 33, 63, 64, 65 and 511 pairwise different candidates (below 512: the matrix path, one stage): the
    winner's support has members on both sides of the seams 15 | 16 and 31 | 32, in the last block and at index c - 1, and
    differs from what the table without its last block gives (test_link_tables_cpu.py).  At t = 12 every size but 32 and 64 has
    zero rows to take out again."""
    got = _check(T.block_case(t, sizes))
    assert [e.opening.candidates for e in got[:len(sizes)]] == list(sizes)


# ---- (c) the dedup path and its limits --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [512, 513])
@pytest.mark.parametrize("t", [10, 12])
def test_dedup_path_with_wrapping_probes(t, c):
    """A hub of 512 or 513 candidates in both regions, 40 distinct hashes: the dedup path at its first sizes, seven of the
    values at home in the table's last two slots, so that their probes wrap to slot 0."""
    got = _check(T.dedup_case(t, c))
    assert got[0].opening.candidates == got[0].ending.candidates == c


@pytest.mark.parametrize("c,distinct", T.LIMITS)
@pytest.mark.parametrize("t", [10, 12])
def test_dedup_limit_and_the_four_stages_behind_it(t, c, distinct):
    """1536 candidates of 1536 distinct hashes: the table exactly at its limit.  1537 of 1536: one duplicate, still deduped.
    1537 of 1537: the matrix path over four stages, the last of one row and 31 zero rows (at t = 12: the pad correction on the
    last stage); the winner's support has members in every stage.  Both regions, a spoke holds one segment in each."""
    got = _check(T.limit_case(t, c, distinct))
    assert got[0].opening.candidates == got[0].ending.candidates == c


# ---- (d) slot edges -----------------------------------------------------------------------------------------------------------------
def test_slots_of_16_17_24_and_25_runs():
    """Behind 40 single spokes, four that share 16, 17 (kOwnCopy: a slot's own thread | the workgroup copies its entries), 24
    and 25 (kEpilogueBucketLimit: a lane | pair_entries_large_kernel orders the bucket) segments with the hub.  Buckets of many
    runs: results against the oracle, evidence against the host definition over the oracle's run list."""
    case = T.slot_case()
    before = capi.epilogue_host_fallbacks()
    corpus = _corpus(case)
    index = _index(corpus)
    assert _as(index.results()) == _oracle(corpus)
    runs = M.oracle_runs(case.rows(), case.t, case.min_len, threads=_threads())
    assert sorted(np.bincount(runs["problem"].astype(np.int64)).tolist())[-4:] == [16, 17, 24, 25]
    cmp = corpus.comparator()
    results, want = cmp.results_from_runs_evidence(corpus.c, runs)
    assert _as(results) == _as(index.results())
    got = index.evidence()
    for v, (g, w) in enumerate(zip(got, want)):
        for name in ("opening", "ending"):
            assert M.same_evidence(getattr(g, name), getattr(w, name)), (v, name, getattr(g, name), getattr(w, name))
    count = T.links(case.tables[0], case.bound)                        # (the order inside a bucket is the heap's: by hash)
    hub = got[0].opening
    assert hub.candidates == sum(T.SLOT_SHARES) and hub.support == count.max() == count[case.tables[0] == hub.match_hash][0]
    assert capi.epilogue_host_fallbacks() == before


# ---- (e) the other video policies -------------------------------------------------------------------------------------------------
POLICY_CASES = [lambda: T.edge_case(10), lambda: T.edge_case(11), lambda: T.edge_case(12),
                lambda: T.block_case(10, (33, 65)), lambda: T.block_case(12, (33, 65))]


@pytest.mark.parametrize("make", POLICY_CASES, ids=["edge-t10", "edge-t11", "edge-t12", "blocks-t10", "blocks-t12"])
def test_library_and_grouped_policies(make, monkeypatch):
    """The same kernel body under the library job's addressing (Comparator.run_with_frame_hashes, device epilogue) and under
    the grouped one (the library twice, as two shows with interleaved labels): results against the oracle."""
    monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", "1")
    case = make()
    before = capi.epilogue_host_fallbacks()
    corpus = _corpus(case)
    want = _oracle(corpus)
    assert _as(corpus.comparator().run_with_frame_hashes(corpus.c)) == want
    twice = _corpus(case, copies=2)
    labels = [7, 0xFFFFFFFF] * len(corpus.c)
    got = _as(twice.comparator().run_with_frame_hashes(twice.c, groups=labels))
    assert got[0::2] == want and got[1::2] == want
    assert any(r is not None and r[0] is not None for r in want[:len(case.tables)])
    assert capi.epilogue_host_fallbacks() == before


def test_library_policy_on_the_dedup_path(monkeypatch):
    monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", "1")
    case = T.dedup_case(10, 513)
    before = capi.epilogue_host_fallbacks()
    corpus = _corpus(case)
    assert _as(corpus.comparator().run_with_frame_hashes(corpus.c)) == _oracle(corpus)
    assert capi.epilogue_host_fallbacks() == before
