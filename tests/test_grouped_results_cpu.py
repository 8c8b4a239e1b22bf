"""CPU: the host definition of a grouped search (needle_hip_comparator_results_from_runs_grouped, csrc/comparator.cpp; the
numbering: csrc/pair_ids.h) against the ORACLE's run_with_frame_hashes over every group's own sub-list, field for field.  The
run lists are the oracle's scan of each group, re-tagged with the grouped pair ids: no device anywhere.  A video's
find_best_match is a pure function of its candidate list in pair order, and restricting the pairs to one group keeps their
relative order -- so the per-group oracle IS the definition, with no checker of its own."""
import numpy as np
import pytest

from needle_amd import capi
from oracle import oracle as O
from tests import best_match_model as M

NS = O.NS
THRESHOLD, MIN_S = 10, 10
INVALID = capi.ERROR_NAMES.index("InvalidArgument")
ALONE = 0x12345678
# interleaved groups: label 7 (4 videos), 0 (3), 0xFFFFFFFF (2), one video alone
LABELS = [7, 0, 7, 0xFFFFFFFF, 0, ALONE, 7, 0xFFFFFFFF, 0, 7]
# (seed, endings, padding in seconds, exact copies)
LIBRARIES = [(201, False, 0.0, False), (202, True, 0.25, False), (203, True, 0.0, True), (204, False, 1.0, True)]


def members_of(labels):
    """groups in order of first appearance -> their list positions, ascending"""
    out = {}
    for v, g in enumerate(labels):
        out.setdefault(g, []).append(v)
    return list(out.values())


def enumerate_pairs(labels):
    """The grouped numbering by enumeration: group after group, i-major over each group's members."""
    return [(m[x], m[y]) for m in members_of(labels) for x in range(len(m)) for y in range(x + 1, len(m))]


def planted_rows(seed, labels, endings, exact, kept=420, short=None):
    """rows[v][r]: random hashes; every group of two or more shares one segment per region (bit-identical copies with
    `exact`: equal simhashes, equal lengths -- ties that only the candidate order breaks), groups of four a second, longer
    one in two of their members.  `short`: a video whose rows hold 20 hashes -- no run of its pairs can be long enough."""
    rng = np.random.default_rng(seed)
    new = lambda k: rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
    regions = 2 if endings else 1
    rows = [[new(20 if v == short else kept) for _ in range(regions)] for v in range(len(labels))]

    def plant(seg, v, r, at):
        if v == short:
            return
        flips = 0 if exact else (np.uint32(1) << rng.integers(0, 32, len(seg)).astype(np.uint32)) * (rng.random(len(seg)) < 0.3)
        rows[v][r][at:at + len(seg)] = seg ^ np.asarray(flips, dtype=np.uint32)

    for m in members_of(labels):
        if len(m) < 2:
            continue
        for r in range(regions):
            seg = new(100 + 10 * r)
            for k, v in enumerate(m):
                plant(seg, v, r, 15 + 23 * k + 40 * r)
            if len(m) >= 4:
                longer = new(130)
                plant(longer, m[1], r, 250)
                plant(longer, m[3], r, 270)
    return rows


class Library:
    def __init__(self, seed, endings, padding, exact, labels=LABELS, short=None):
        self.labels, self.endings, self.padding = list(labels), endings, padding
        self.rows = planted_rows(seed, labels, endings, exact, short=short)
        self.ts = M.timestamps(self.rows)
        self.n = len(self.rows)
        pairs = lambda v, r: list(zip(self.rows[v][r].tolist(), self.ts[v][r]))
        self.c = [capi.FrameHashes.new(pairs(v, 0), pairs(v, 1) if endings else [], M.HD) for v in range(self.n)]
        self.o = [O.FrameHashes(pairs(v, 0), pairs(v, 1) if endings else [], M.HD) for v in range(self.n)]
        self.cmp = capi.Comparator([f"v{k}.mkv" for k in range(self.n)], include_endings=endings, hash_match_threshold=THRESHOLD,
                                   min_opening_duration=MIN_S, min_ending_duration=MIN_S, time_padding=padding)
        self.oracle_cmp = O.Comparator(include_endings=endings, hash_match_threshold=THRESHOLD, min_opening_duration=MIN_S * NS,
                                       min_ending_duration=MIN_S * NS, time_padding=O.duration_from_secs_f32(padding))
        self.regions = 2 if endings else 1
        self.pair_ids = {tuple(p): k for k, p in enumerate(capi.group_pairs(self.labels).tolist())}
        self.runs = self.grouped_runs()

    def grouped_runs(self):
        """Every group's own all-pairs run list from the oracle's scan, its local i-major pair turned into the grouped id."""
        parts = []
        for m in members_of(self.labels):
            if len(m) < 2:
                continue
            runs = M.oracle_runs([self.rows[v] for v in m], THRESHOLD, M.min_len_for(MIN_S))
            local = [(i, j) for i in range(len(m)) for j in range(i + 1, len(m))]
            for k in range(len(runs)):
                i, j = local[int(runs["problem"][k]) // self.regions]
                runs["problem"][k] = self.pair_ids[(m[i], m[j])] * self.regions + int(runs["problem"][k]) % self.regions
            parts.append(runs)
        return np.concatenate(parts) if parts else np.zeros(0, dtype=capi.RUN_DTYPE)

    def oracle_per_group(self):
        want = [None] * self.n
        for m in members_of(self.labels):
            for v, r in zip(m, O.run_with_frame_hashes(self.oracle_cmp, [self.o[v] for v in m])):
                want[v] = r
        return want


def _as(rs):
    return [None if r is None else (r.opening, r.ending) for r in rs]


@pytest.fixture(scope="module", params=LIBRARIES, ids=lambda p: f"seed{p[0]}-endings{int(p[1])}-pad{p[2]}-exact{int(p[3])}")
def library(request):
    return Library(*request.param)


def test_group_pairs_is_the_enumeration():
    """needle_hip_group_pairs against the enumeration tests/cpp/group_ids_check.cpp checks the header with."""
    big = [0xFFFFFFFF if v % 9 else v // 9 % 3 for v in range(290)]         # one group of 257 between three small ones
    for labels in (LABELS, [5], [], [3, 3], [1, 2, 3], [0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0], big):
        got = capi.group_pairs(labels)
        assert got.shape == (len(enumerate_pairs(labels)), 2) and got.tolist() == [list(p) for p in enumerate_pairs(labels)]
    n = 9
    one = capi.group_pairs([42] * n).tolist()                                # one group: the comparator's i-major order
    assert one == [[i, j] for i in range(n) for j in range(i + 1, n)]
    count = capi.C.c_uint64(0)                                               # a short buffer gets the first pairs, the count stays
    some = np.full((3, 2), 77, dtype=np.uint32)
    labels = np.asarray(LABELS, dtype=np.uint32)
    assert capi.lib().needle_hip_group_pairs(labels.ctypes.data, labels.size, some.ctypes.data, 2, capi.C.byref(count)) == 0
    assert count.value == len(enumerate_pairs(LABELS)) and some.tolist() == [list(p) for p in enumerate_pairs(LABELS)[:2]] + [[77, 77]]


def test_grouped_results_equal_the_oracle_per_group(library):
    assert len(library.runs) >= 6 + 3 + 1, "every planted pair has its run"
    got = _as(library.cmp.results_from_runs_grouped(library.c, library.labels, library.runs))
    want = _as(library.oracle_per_group())
    for v in range(library.n):
        print(v, library.labels[v], got[v], want[v])
    assert got == want
    alone = library.labels.index(ALONE)
    assert got[alone] is None
    assert all(got[v] is not None and got[v][0] is not None for v in range(library.n) if v != alone)
    if library.endings:
        assert all(got[v][1] is not None for v in range(library.n) if v != alone)
    shuffled = library.runs[np.random.default_rng(1).permutation(len(library.runs))]   # the list's order says nothing
    assert _as(library.cmp.results_from_runs_grouped(library.c, library.labels, shuffled)) == want


def test_a_video_with_rows_too_short_has_no_run_and_changes_nobody(library):
    """Video 4 (group 0) with 20 hashes a row: its pairs hold no run; the others of its group still find each other."""
    lib = Library(300 + library.n, library.endings, library.padding, False, short=4)
    got = _as(lib.cmp.results_from_runs_grouped(lib.c, lib.labels, lib.runs))
    assert got == _as(lib.oracle_per_group())
    assert got[4] is None and got[1] is not None and got[8] is not None


def test_one_group_is_the_ungrouped_call(library):
    """All videos under one label: the run list of the ungrouped numbering, the ungrouped results -- cross-season matches and all."""
    runs = M.oracle_runs(library.rows, THRESHOLD, M.min_len_for(MIN_S))
    old = _as(library.cmp.results_from_runs(library.c, runs))
    for label in (0, 0xFFFFFFFF, 31):
        assert _as(library.cmp.results_from_runs_grouped(library.c, [label] * library.n, runs)) == old
    assert old == _as(O.run_with_frame_hashes(library.oracle_cmp, library.o))
    assert old[library.labels.index(ALONE)] is None


def test_refusals(library):
    n, L = library.n, capi.lib()
    arr = (capi.C.c_void_p * n)(*[f._h for f in library.c])
    res = (capi.CSearchResult * n)()
    labels = np.asarray(library.labels, dtype=np.uint32)
    h = library.cmp.handle()
    call = lambda runs: L.needle_hip_comparator_results_from_runs_grouped(h, arr, n, labels.ctypes.data, runs.ctypes.data, runs.size, res)
    assert call(library.runs) == 0
    beyond = library.runs.copy()
    beyond["problem"][len(beyond) // 2] = len(library.pair_ids) * library.regions     # the first problem the groups do not have
    assert call(beyond) == INVALID
    with pytest.raises(capi.NeedleError, match="names problem") as e:
        library.cmp.results_from_runs_grouped(library.c, library.labels, beyond)
    assert e.value.code == INVALID
    beyond["problem"][len(beyond) // 2] = 0xFFFFFFFF
    assert call(beyond) == INVALID
    null = capi.ERROR_NAMES.index("NullArgument")
    assert L.needle_hip_comparator_results_from_runs_grouped(h, arr, n, labels.ctypes.data, None, 3, res) == null
    assert L.needle_hip_comparator_results_from_runs_grouped(h, arr, n, labels.ctypes.data, library.runs.ctypes.data, library.runs.size, None) == null
    assert L.needle_hip_comparator_results_from_runs_grouped(None, arr, n, labels.ctypes.data, library.runs.ctypes.data, library.runs.size, res) == null
    count = capi.C.c_uint64(0)
    assert L.needle_hip_group_pairs(labels.ctypes.data, n, None, 0, None) == null
    assert L.needle_hip_group_pairs(None, n, None, 0, capi.C.byref(count)) == null
    with pytest.raises(ValueError):
        library.cmp.results_from_runs_grouped(library.c, library.labels[:-1], library.runs)


def test_a_missing_ending_matters_only_to_a_video_that_has_a_pair():
    lib = Library(205, True, 0.0, False)
    pairs = lambda v: list(zip(lib.rows[v][0].tolist(), lib.ts[v][0]))
    alone, paired = lib.labels.index(ALONE), lib.labels.index(0xFFFFFFFF)
    fhs = list(lib.c)
    fhs[alone] = capi.FrameHashes.new(pairs(alone), [], M.HD)                 # nobody compares it: no error, same results
    assert _as(lib.cmp.results_from_runs_grouped(fhs, lib.labels, lib.runs)) == _as(lib.oracle_per_group())
    fhs[paired] = capi.FrameHashes.new(pairs(paired), [], M.HD)               # one of a group of two
    with pytest.raises(capi.NeedleError, match="no ending hash data present"):
        lib.cmp.results_from_runs_grouped(fhs, lib.labels, lib.runs)
