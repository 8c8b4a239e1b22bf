"""CPU: the host definition of match evidence (needle_hip_comparator_results_from_runs_evidence, csrc/comparator.cpp) against
the NumPy model of tests/best_match_model.py, over planted libraries whose runs and simhashes come from the oracle's scan.
The results the new call writes are the old call's, the evidence agrees with the oracle's full search through the two
equations of needle_hip.h, a video or region without a match reads UINT32_MAX / zeros, and the refusals are the old call's."""
import ctypes as C

import numpy as np
import pytest

from needle_amd import capi
from oracle import oracle as O
from tests import best_match_model as M

NS = O.NS
THRESHOLD, MIN_S = 10, 10
NULL_ARGUMENT, INVALID = capi.ERROR_NAMES.index("NullArgument"), capi.ERROR_NAMES.index("InvalidArgument")
# (seed, endings, padding in seconds): seeds for which the oracle's run list alone satisfies the model's precondition
LIBRARIES = [(101, False, 0.0), (102, True, 0.25), (103, True, 0.0)]


class Library:
    def __init__(self, seed, endings, padding, lonely=True):
        self.endings, self.padding = endings, padding
        self.rows = M.planted_library(seed, endings)
        if lonely:                                       # a seventh video that shares nothing: no result at all
            rng = np.random.default_rng(seed + 1000)
            self.rows.append([rng.integers(0, 2 ** 32, 600, dtype=np.uint64).astype(np.uint32) for _ in self.rows[0]])
        self.ts = M.timestamps(self.rows)
        self.n = len(self.rows)
        pairs = lambda v, r: list(zip(self.rows[v][r].tolist(), self.ts[v][r]))
        self.c = [capi.FrameHashes.new(pairs(v, 0), pairs(v, 1) if endings else [], M.HD) for v in range(self.n)]
        self.o = [O.FrameHashes(pairs(v, 0), pairs(v, 1) if endings else [], M.HD) for v in range(self.n)]
        self.runs = M.oracle_runs(self.rows, THRESHOLD, M.min_len_for(MIN_S))
        self.cmp = capi.Comparator([f"v{k}.mkv" for k in range(self.n)], include_endings=endings, hash_match_threshold=THRESHOLD,
                                   min_opening_duration=MIN_S, min_ending_duration=MIN_S, time_padding=padding)
        self.pad_ns = O.duration_from_secs_f32(padding)
        self.oracle_cmp = O.Comparator(include_endings=endings, hash_match_threshold=THRESHOLD, min_opening_duration=MIN_S * NS,
                                       min_ending_duration=MIN_S * NS, time_padding=self.pad_ns)


@pytest.fixture(scope="module", params=LIBRARIES, ids=lambda p: f"seed{p[0]}-endings{int(p[1])}-pad{p[2]}")
def library(request):
    return Library(*request.param)


def test_symbols_and_layout():
    L = capi.lib()
    assert hasattr(L, "needle_hip_comparator_results_from_runs_evidence") and hasattr(L, "needle_hip_index_evidence")
    assert C.sizeof(capi.CMatchEvidence) == 72 and C.sizeof(capi.CSearchEvidence) == 144
    assert capi.CMatchEvidence.score.offset == 24 and capi.CMatchEvidence.start_ns.offset == 40


def test_host_evidence_equals_the_model(library):
    M.assert_one_run_per_bucket(library.runs)            # the precondition, on the oracle's list
    assert len(library.runs) >= 9 + (3 if library.endings else 0), "every planted pair has its run"
    results, evidence = library.cmp.results_from_runs_evidence(library.c, library.runs)
    want_res, want_ev = M.evidence_model(library.ts, library.runs, THRESHOLD, (MIN_S * NS, MIN_S * NS), library.endings, library.pad_ns)
    for v in range(library.n):
        for which, name in enumerate(("opening", "ending")):
            got = getattr(evidence[v], name)
            print(v, name, got)
            assert M.same_evidence(got, want_ev[v][which]), (v, name, got, want_ev[v][which])
        assert (None if results[v] is None else (results[v].opening, results[v].ending)) == want_res[v], v
    # what the plants mean (at least: threshold + threshold / 2 = 15 of 32 bits also lets unrelated simhashes agree): videos
    # 0-2 hold the first opening only, with three partners each, 4 and 5 the second, longer one, video 3 both
    for v in (0, 1, 2):
        assert evidence[v].opening.partners >= 3 and evidence[v].opening.support >= 3 and evidence[v].opening.partner in (0, 1, 2, 3)
    for v in (4, 5):
        assert evidence[v].opening.partners >= 2 and evidence[v].opening.partner in (3, 4, 5)
    assert evidence[3].opening.candidates >= 5 and evidence[3].opening.partner in (4, 5), "video 3 holds both: the longer one wins"
    for v in range(library.n - 1):
        assert evidence[v].opening.partners <= evidence[v].opening.support <= evidence[v].opening.candidates
    if library.endings:
        assert evidence[5].ending.partners >= 2 and evidence[5].ending.partner in (1, 4) and evidence[5].ending.is_source is False
        assert evidence[0].ending is None and evidence[0].opening is not None


def test_evidence_is_consistent_with_the_oracles_results(library):
    want = O.run_with_frame_hashes(library.oracle_cmp, library.o)
    _, evidence = library.cmp.results_from_runs_evidence(library.c, library.runs)
    matched = 0
    for v in range(library.n):
        for name in ("opening", "ending"):
            ev = getattr(evidence[v], name)
            res = None if want[v] is None else getattr(want[v], name)
            assert (ev is None) == (res is None), (v, name)
            if ev is not None:
                assert res[0] == ev.interval[0] + library.pad_ns
                assert res[1] == ev.interval[1] - library.pad_ns - M.HD
                matched += 1
    assert matched >= 6 + (3 if library.endings else 0)


def test_threshold_zero_nobody_links_and_the_model_skips_them():
    """t = 0: bound = 0, no candidate is within it of any other or of itself, and find_best_match skips a candidate without
    links (comparator.rs `count == 0`): a video with candidates has a result with neither side.  The model against the oracle's
    full search, and the host definition's evidence against the model's."""
    from tests import link_tables as T
    case = T.edge_case(0, rotations=2)
    rows = case.rows()
    ts = M.timestamps(rows)
    pairs = lambda v, r: list(zip(rows[v][r].tolist(), ts[v][r]))
    c = [capi.FrameHashes.new(pairs(v, 0), [], M.HD) for v in range(len(rows))]
    o = [O.FrameHashes(pairs(v, 0), [], M.HD) for v in range(len(rows))]
    runs = M.oracle_runs(rows, 0, case.min_len)
    assert len(runs) == 32, "two hubs of sixteen exact copies"
    want = O.run_with_frame_hashes(O.Comparator(hash_match_threshold=0, min_opening_duration=case.min_s * NS), o)
    assert all(r is not None and r.opening is None and r.ending is None for r in want)
    model_res, model_ev = M.evidence_model(ts, runs, 0, (case.min_s * NS, case.min_s * NS), False)
    assert model_res == [(None, None)] * len(rows) and model_ev == [(None, None)] * len(rows)
    cmp = capi.Comparator([f"v{k}.mkv" for k in range(len(rows))], hash_match_threshold=0, min_opening_duration=case.min_s)
    results, evidence = cmp.results_from_runs_evidence(c, runs)
    assert [(r.opening, r.ending) for r in results] == model_res
    assert all(e.opening is None and e.ending is None for e in evidence)


def test_no_match_reads_uint32_max_and_zeros(library):
    n = library.n
    arr = (C.c_void_p * n)(*[f._h for f in library.c])
    ev = (capi.CSearchEvidence * n)()
    C.memset(ev, 0x5A, C.sizeof(ev))
    assert capi.lib().needle_hip_comparator_results_from_runs_evidence(library.cmp.handle(), arr, n, library.runs.ctypes.data,
                                                                       library.runs.size, 0, n, None, ev) == 0
    none = bytes([0xFF] * 4) + bytes(C.sizeof(capi.CMatchEvidence) - 4)
    lonely = ev[n - 1]                                   # shares nothing with anybody: no result, no evidence
    assert bytes(lonely.opening) == none and bytes(lonely.ending) == none
    if not library.endings:
        assert all(bytes(ev[v].ending) == none for v in range(n)), "without include_endings the ending half is always that"
    else:
        assert bytes(ev[0].ending) == none and bytes(ev[0].opening) != none
    assert all(ev[v].opening.reserved == 0 and ev[v].ending.reserved == 0 for v in range(n))


def test_results_are_the_old_calls_byte_for_byte(library):
    n = library.n
    arr = (C.c_void_p * n)(*[f._h for f in library.c])
    for first, count in ((0, n), (2, 3), (n, 0)):
        old, new = (capi.CSearchResult * n)(), (capi.CSearchResult * n)()
        C.memset(old, 0xA5, C.sizeof(old))
        C.memset(new, 0x3C, C.sizeof(new))
        ev = (capi.CSearchEvidence * n)()
        h = library.cmp.handle()
        assert capi.lib().needle_hip_comparator_results_from_runs(h, arr, n, library.runs.ctypes.data, library.runs.size, first, count, old) == 0
        assert capi.lib().needle_hip_comparator_results_from_runs_evidence(h, arr, n, library.runs.ctypes.data, library.runs.size, first,
                                                                           count, new, ev) == 0
        assert bytes(old) == bytes(new), (first, count)
        for v in range(n):                               # a slot outside the block is left empty, as its result is
            if not first <= v < first + count:
                assert ev[v].opening.partner == capi.NO_PARTNER and ev[v].ending.partner == capi.NO_PARTNER


def test_refusals_are_the_old_calls(library):
    n = library.n
    L = capi.lib()
    h = library.cmp.handle()
    arr = (C.c_void_p * n)(*[f._h for f in library.c])
    holed = (C.c_void_p * n)(*[f._h for f in library.c])
    holed[2] = None
    res, ev = (capi.CSearchResult * n)(), (capi.CSearchEvidence * n)()
    runs, k = library.runs.ctypes.data, library.runs.size
    cases = [(None, arr, n, runs, k, 0, n), (h, None, n, runs, k, 0, n), (h, arr, n, None, k, 0, n), (h, holed, n, runs, k, 0, n),
             (h, arr, n, runs, k, n + 1, 0), (h, arr, n, runs, k, 1, n), (h, arr, n, None, 0, 0, n)]
    codes = []
    for args in cases:
        old = L.needle_hip_comparator_results_from_runs(*args, res)
        new = L.needle_hip_comparator_results_from_runs_evidence(*args, res, ev)
        assert old == new, args
        codes.append(new)
    assert codes == [NULL_ARGUMENT, NULL_ARGUMENT, NULL_ARGUMENT, NULL_ARGUMENT, INVALID, INVALID, 0]
    assert L.needle_hip_comparator_results_from_runs_evidence(h, arr, n, runs, k, 0, n, res, None) == NULL_ARGUMENT
    # the index's call, as far as it goes without a device
    assert L.needle_hip_index_evidence(None, ev, n) == NULL_ARGUMENT
