"""CPU: the hub libraries of tests/link_tables.py are what they claim to be, before tests/test_gpu_link_counts.py runs them
through best_match_kernel.  For every case: the oracle's scan finds exactly the planted runs and no other, the hub's candidate
hashes are the targets in order, the model of tests/best_match_model.py agrees with the oracle's full search on results and
with the host definition (needle_hip_comparator_results_from_runs_evidence) on evidence, and the hub's (winner, support)
computed from the targets alone is the model's.  Every edge table proves that the bound decides something: under bound - 1,
bound and bound + 1 the hub's (winner, support) are pairwise different, at every rotation; every block table that dropping the
last block changes it; the collide palettes that their probes wrap.  Seeds are fixed in link_tables.py."""
import os

import numpy as np
import pytest

from needle_amd import capi
from oracle import oracle as O
from tests import best_match_model as M
from tests import link_tables as T

NS = O.NS
EDGE_T = (0, 1, 2, 10, 11, 12, 14)


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


class Library:
    """A case's rows as both sides' FrameHashes, with the oracle's run list."""

    def __init__(self, case):
        self.case = case
        self.rows = case.rows()
        self.ts = M.timestamps(self.rows)
        self.n = len(self.rows)
        pairs = lambda v, r: list(zip(self.rows[v][r].tolist(), self.ts[v][r]))
        self.c = [capi.FrameHashes.new(pairs(v, 0), pairs(v, 1) if case.endings else [], M.HD) for v in range(self.n)]
        self.o = [O.FrameHashes(pairs(v, 0), pairs(v, 1) if case.endings else [], M.HD) for v in range(self.n)]
        self.runs = M.oracle_runs(self.rows, case.t, case.min_len, threads=_threads())
        self.cmp = capi.Comparator([f"v{k}.mkv" for k in range(self.n)], include_endings=case.endings, hash_match_threshold=case.t,
                                   min_opening_duration=case.min_s, min_ending_duration=case.min_s)
        self.oracle_cmp = O.Comparator(include_endings=case.endings, hash_match_threshold=case.t,
                                       min_opening_duration=case.min_s * NS, min_ending_duration=case.min_s * NS)


CASES = [T.edge_case(t) for t in EDGE_T] + [T.block_case(t, sizes) for t in (10, 12) for sizes in T.BLOCK_SIZES] + \
    [T.dedup_case(t, c) for t in (10, 12) for c in (512, 513)] + [T.limit_case(12, 1537, 1537), T.slot_case()]


@pytest.fixture(scope="module", params=CASES, ids=repr)
def library(request):
    return Library(request.param)


def _as(rs):
    return [None if r is None else (r.opening, r.ending) for r in rs]


def test_simhash_is_the_oracles():
    rng = np.random.default_rng(1)
    for k in (1, 2, 3, 22, 23):
        rows = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
        assert T.simhash(rows) == O.simhash32(rows)
    assert T.simhash(np.array([0xFFFF0000, 0x0000FFFF], dtype=np.uint32)) == 0, "a tie clears the bit"


def test_the_oracle_finds_exactly_the_planted_runs(library):
    case, runs = library.case, library.runs
    got = sorted(zip(runs["problem"].tolist(), runs["src_end"].tolist(), runs["dst_end"].tolist(), runs["len"].tolist()))
    want = case.planted()
    unplanned, missed = sorted(set(got) - set(want)), sorted(set(want) - set(got))
    assert len(unplanned) == 0 and len(missed) == 0, (unplanned[:5], missed[:5])
    assert len(got) == len(want) == sum(len(tb) for tb in case.tables)
    crowd = np.bincount(runs["problem"].astype(np.int64)).max()
    assert crowd <= (case.per_spoke if isinstance(case.per_spoke, int) else max(case.per_spoke))
    assert (crowd == 1) == case.one_run_per_bucket
    # the hub's candidate hashes, in candidate order (pair, then region), are the targets
    regions, n = (2 if case.endings else 1), library.n
    if case.one_run_per_bucket:
        order = np.argsort(runs["problem"], kind="stable")
        for h, table in enumerate(case.tables):
            lo = (h * n - h * (h + 1) // 2) * regions                 # hub h's pairs as a source: a contiguous block of problems
            hi = lo + (n - h - 1) * regions
            mine = runs[order][(runs["problem"][order] >= lo) & (runs["problem"][order] < hi)]
            assert mine["src_match_hash"].tolist() == table.tolist(), h
    else:                                                             # (several runs a bucket: the order inside one is the heap's)
        assert sorted(runs["src_match_hash"].tolist()) == sorted(case.tables[0].tolist())


def test_model_oracle_and_host_definition_agree(library):
    case = library.case
    want = _as(O.run_with_frame_hashes(library.oracle_cmp, library.o, threads=_threads()))
    results, evidence = library.cmp.results_from_runs_evidence(library.c, library.runs)
    assert _as(results) == want
    if not case.one_run_per_bucket:
        return
    min_ns = (case.min_s * NS, case.min_s * NS)
    model_res, model_ev = M.evidence_model(library.ts, library.runs, case.t, min_ns, case.endings)
    assert model_res == want
    for v in range(library.n):
        for which, name in enumerate(("opening", "ending")):
            assert M.same_evidence(getattr(evidence[v], name), model_ev[v][which]), (v, name)
    for h, table in enumerate(case.tables):                           # the targets alone say who wins and with how many links
        got = tuple(None if e is None else (e.candidate, e.support) for e in model_ev[h])
        assert got == case.winners(h), (h, got)
        if case.bound == 0:
            assert want[h] == (None, None), "nobody links: a result with neither side"


@pytest.mark.parametrize("t", EDGE_T)
def test_edge_tables_prove_themselves(t):
    case = T.edge_case(t)
    b = case.bound
    table = T.edge_table(t)
    for h in range(16):
        if b == 0:
            assert case.winners(h) == (None, None) and case.winners(h, 1)[0] is not None
            continue
        seen = [case.winners(h, bound)[0] if bound > 0 else None for bound in (b - 1, b, b + 1)]
        assert len(set(seen)) == 3, (t, h, seen)
    assert [case.tables[h].tolist() for h in range(16)] == [np.roll(table, -h).tolist() for h in range(16)], \
        "every member visits every position of a half tile"


@pytest.mark.parametrize("t", [10, 12])
def test_block_tables_prove_themselves(t):
    case = T.block_case(t, sum(T.BLOCK_SIZES, ()))
    for h, table in enumerate(case.tables):
        c = len(table)
        assert len(np.unique(table)) == c
        w, support = case.winners(h)[0]
        near = T.popcount(table ^ table[w]) < case.bound
        assert support == near.sum() and all(near[p] for p in T.seam_positions(c)), "the support straddles every seam"
        last_block = (c - 1) // 32 * 32
        if last_block:                                                # a last block dropped, or miscounted by its members
            assert near[last_block:].any() and T.winner(table[:last_block], True, case.bound)[0] != (w, support), c


@pytest.mark.parametrize("t", [10, 12])
def test_limit_tables_prove_themselves(t):
    for c, distinct in T.LIMITS:
        case = T.limit_case(t, c, distinct)
        table = case.tables[0]
        assert len(table) == c and len(np.unique(table)) == distinct
        for w, support in case.winners(0):
            near = T.popcount(table ^ table[w]) < case.bound
            per_stage = [int(near[lo:lo + 512].sum()) for lo in range(0, c, 512)]
            assert min(per_stage) >= 1 and sum(per_stage) == support, "a stage lost or counted twice changes the support"
            assert all(near[p] for p in T.seam_positions(c))


@pytest.mark.parametrize("t", [10, 12])
def test_collide_palettes_wrap_past_the_last_slot(t):
    """What `sl + 1` in place of `(sl + 1) & (kSlots - 1)` would do, on the table model (not a thing to try on a device: it
    reads beyond the table): seven keys whose home slots are 2046 and 2047 take slots 0 .. 4 -- without the wrap, 2048 .. 2052."""
    for table in (T.dedup_case(t, c).tables[0] for c in (512, 513)):
        assert len(np.unique(table)) == 40
        wrapped, unwrapped = T.table_slots(table), T.table_slots(table, wrap=False)
        assert max(wrapped.values()) == T.SLOTS - 1 and {0, 1, 2, 3, 4} <= set(wrapped.values())
        assert max(unwrapped.values()) == T.SLOTS + 4, "the probes run five slots past the table"
        moved = [h for h in wrapped if wrapped[h] != unwrapped[h]]
        assert len(moved) >= 5 and all(int(T.home_slot(h)) >= T.SLOTS - 2 or wrapped[h] <= 8 for h in moved)
