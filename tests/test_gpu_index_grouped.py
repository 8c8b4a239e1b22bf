"""-m gpu: the grouped incremental index (capi.Index(comparator, grouped=True): needle_hip_index_new_grouped / _add_grouped /
_groups; the append-stable numbering: needle_amd/csrc/pair_ids.h IndexGroupView; the kernels under it: epilogue_kernels.h and
index_store.hip).  After every operation the index's results are compared, to the nanosecond, with the ORACLE's
run_with_frame_hashes over every group's own sub-list of the current list, and with Comparator.run_with_frame_hashes(groups=...)
over the current list under both of its epilogues (NEEDLE_HIP_DEVICE_EPILOGUE=0 and =1: the flag is the comparator's; the index
has one form, and its host fallback is forced as tests/test_gpu_index_evidence.py forces it).  Videos are planted as
tests/test_gpu_grouped.py plants them: rows of a few hundred random hashes with shared segments written in; 246 ms a hash,
minimum durations of 5-20 s."""
import numpy as np
import pytest

from needle_amd import capi
from oracle import oracle as O
from tests import best_match_model as M
from tests.test_gpu_feeder_formats import timed
from tests.test_gpu_grouped import FORMS, HD, Videos, _as, even_timestamps, members_of, random_rows

pytestmark = pytest.mark.gpu
NS = O.NS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _new(rng, k):
    return rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)


class Live:
    """A grouped index and the list it stands for (ids into a pool of videos, and their labels): every operation is applied
    to both, then checked.  The oracle's answer for a group's sub-list is computed once per sub-list."""

    def __init__(self, pool, labels, monkeypatch, min_s, padding=0.0, evidence=True):
        self.pool, self.pool_labels, self.monkeypatch = pool, labels, monkeypatch
        self.min_s, self.padding, self.evidence = min_s, padding, evidence
        self.cmp, self.ocmp = pool.comparators(min_s=min_s, padding=padding)
        self.index = capi.Index(self.cmp, grouped=True)
        self.cur, self.labels, self.total, self.known, self.known_evidence = [], [], 0, {}, {}

    # ---- what the current list should give
    def _group_results(self, ids):
        if ids not in self.known:
            self.known[ids] = _as(O.run_with_frame_hashes(self.ocmp, [self.pool.o[p] for p in ids], threads=8))
        return self.known[ids]

    def expect(self):
        want = [None] * len(self.cur)
        for m in members_of(self.labels):
            for v, r in zip(m, self._group_results(tuple(self.cur[v] for v in m))):
                want[v] = r
        return want

    def expect_evidence(self):
        """needle_hip_comparator_results_from_runs_evidence per group over the oracle's run list of that group's sub-list, the
        partner mapped back to list positions."""
        none = capi.SearchEvidence(None, None)
        want = [none] * len(self.cur)
        regions = 2 if self.pool.endings else 1
        for m in members_of(self.labels):
            if len(m) < 2:
                continue                                                   # alone in its group: no pair, partner = UINT32_MAX
            ids = tuple(self.cur[v] for v in m)
            if ids not in self.known_evidence:
                rows = [[self.pool.rows[p][r] for r in range(regions)] for p in ids]
                runs = M.oracle_runs(rows, 10, M.min_len_for(self.min_s), threads=8)
                host = capi.Comparator([f"v{k}.mkv" for k in range(len(ids))], include_endings=self.pool.endings, hash_match_threshold=10,
                                       min_opening_duration=self.min_s, min_ending_duration=self.min_s, time_padding=self.padding)
                results, evidence = host.results_from_runs_evidence([self.pool.c[p] for p in ids], runs)
                assert _as(results) == self._group_results(ids)
                self.known_evidence[ids] = evidence
            for v, ev in zip(m, self.known_evidence[ids]):
                want[v] = ev
        return want, members_of(self.labels)

    def check(self, last):
        n = len(self.cur)
        want = self.expect()
        assert len(self.index) == n and self.index.groups() == self.labels
        assert _as(self.index.results()) == want, f"list {self.cur} labels {self.labels}"
        for form in FORMS:
            self.monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", form)
            if n:
                assert _as(self.cmp.run_with_frame_hashes([self.pool.c[p] for p in self.cur], groups=self.labels)) == want, form
        self.monkeypatch.delenv("NEEDLE_HIP_DEVICE_EPILOGUE")
        assert self.index.pairs_searched() == (self.total, last)
        assert self.index.pairs_scanned() == (self.total, last)
        for m in members_of(self.labels):
            if len(m) == 1:
                assert want[m[0]] is None, "a video alone in its group has no result"
        if self.evidence:
            self.check_evidence()

    def check_evidence(self):
        got = self.index.evidence()
        want, groups = self.expect_evidence()
        assert len(got) == len(want)
        for m in groups:
            for v in m:
                for name in ("opening", "ending"):
                    g, w = getattr(got[v], name), getattr(want[v], name)
                    if w is None:
                        assert g is None, (v, name, g)                   # (partner = UINT32_MAX reads as None)
                        continue
                    assert g is not None and g.partner in m and g.partner != v, "a partner is a current position of the same group"
                    assert g.partner == m[w.partner], (v, name)          # the group's sub-list position -> the list position
                    fields = ("is_source", "candidate", "candidates", "support", "partners", "match_hash", "partner_hash", "interval",
                              "partner_interval")
                    assert all(getattr(g, f) == getattr(w, f) for f in fields), (v, name, g, w)
                    assert np.float32(g.score).tobytes() == np.float32(w.score).tobytes()

    def check_store(self):
        """The invariants of tests/test_gpu_index_edit.py after an edit: no dead entry slot, the arena equal to the current rows."""
        held, slots, hashes, ts = self.index.store_sizes()
        assert held == slots, "dead entry slots after an edit"
        assert hashes == sum(len(row) for p in self.cur for row in self.pool.rows[p] if len(row))
        assert ts <= hashes

    # ---- the operations
    def add(self, ids):
        ranks = 0
        for p in ids:                                                      # every row here can hold a run: every pair is searched
            ranks += self.labels.count(self.pool_labels[p])
            self.cur.append(p)
            self.labels.append(self.pool_labels[p])
        fallbacks = capi.epilogue_host_fallbacks()
        self.index.add([self.pool.c[p] for p in ids], groups=[self.pool_labels[p] for p in ids])
        self.fallbacks = capi.epilogue_host_fallbacks() - fallbacks   # (the index's own: check() runs the comparator too)
        self.total += ranks
        self.check(ranks)

    def remove(self, positions):
        self.index.remove(positions)
        self.cur = [p for q, p in enumerate(self.cur) if q not in set(positions)]
        self.labels = [g for q, g in enumerate(self.labels) if q not in set(positions)]
        self.check(0)
        self.check_store()

    def replace(self, positions, ids):
        fallbacks = capi.epilogue_host_fallbacks()
        self.index.replace(positions, [self.pool.c[p] for p in ids])
        self.fallbacks = capi.epilogue_host_fallbacks() - fallbacks
        for q, p in zip(positions, ids):
            self.cur[q] = p                                                # (the label of the position stays)
        last = sum(self.labels.count(self.labels[q]) - 1 for q in positions)   # distinct groups here: no pair counted twice
        self.total += last
        self.check(last)
        self.check_store()

    def state(self):
        return (len(self.index), self.index.groups(), _as(self.index.results()), self.index.pairs_searched(), self.index.pairs_scanned(),
                self.index.store_sizes())


A, B, C2, ALONE = 0xFFFFFFFF, 0, 77, 5
LABELS12 = [A, B, A, C2, B, A, ALONE, B, A, C2, B, A]


def _library_of_four_groups(at0=20, extra=0, kept=600):
    """The 12-video, 4-group interleaved library of test_gpu_grouped.py's test_no_match_crosses_a_group_and_ungrouped_one_does
    (5, 4, 2 and one alone; videos 0 and 1, of different groups, share a segment of ~60 s, longer than either group's ~30 s),
    and `extra` more videos that hold every group's segment (candidates for appends and replacements)."""
    rng = np.random.default_rng(11)
    rows = random_rows(rng, [kept + 7 * v for v in range(12 + extra)])
    segs = {}
    for label, at in ((A, at0), (B, at0 + 40), (C2, at0 + 80)):
        segs[label] = (_new(rng, 122), at)
        for k, v in enumerate(members_of(LABELS12)[[A, B, C2].index(label)]):
            rows[v][0][at + 9 * k: at + 9 * k + 122] = segs[label][0]
    cross = _new(rng, 244)
    rows[0][0][at0 + 280:at0 + 280 + 244] = cross
    rows[1][0][at0 + 310:at0 + 310 + 244] = cross
    return rows, segs


def _plant_extra(rows, segs, v, label, k):
    seg, at = segs[label]
    rows[v][0][at + 9 * k: at + 9 * k + len(seg)] = seg


# ---- 1. isolation with teeth -------------------------------------------------------------------------------------------------
def test_appends_never_cross_a_group_and_a_plain_index_does(monkeypatch):
    """Three appends of uneven size that split every group across appends.  The segment videos 0 and 1 share is never reported
    by the grouped index and always by a plain one over the same list; the video alone in its group has no result; an append
    searches the arriving videos' ranks, not n (n - 1) / 2 pairs."""
    rows, _ = _library_of_four_groups()
    pool = Videos(rows, even_timestamps(rows))
    live = Live(pool, LABELS12, monkeypatch, min_s=20)
    live.add([0, 1, 2, 3, 4])            # ranks 0 0 1 0 1
    assert live.index.pairs_searched() == (2, 2)
    live.add([5, 6])                     # 2 0
    assert live.index.pairs_searched() == (4, 2)
    live.add([7, 8, 9, 10, 11])          # 2 3 1 3 4
    assert live.index.pairs_searched() == (17, 13) and 17 == 10 + 6 + 1 < 12 * 11 // 2
    got = _as(live.index.results())
    assert got[6] is None and all(got[v] is not None and got[v][0] is not None for v in range(12) if v != 6)
    plain = capi.Index(live.cmp)
    plain.add(pool.c[:5])
    plain.add(pool.c[5:7])
    plain.add(pool.c[7:])
    ungrouped = _as(plain.results())
    assert ungrouped == _as(O.run_with_frame_hashes(live.ocmp, pool.o, threads=8))
    for v in (0, 1):                     # the case has teeth: all pairs answer otherwise
        assert ungrouped[v][0] != got[v][0] and ungrouped[v][0][1] - ungrouped[v][0][0] > 50 * NS > got[v][0][1] - got[v][0][0]
    assert plain.pairs_searched() == (66, 45)


# ---- 2. an append that grows an early group ---------------------------------------------------------------------------------------
def test_growing_the_first_group_leaves_the_later_groups_where_they_are(monkeypatch):
    """Three groups; one more video joins the FIRST.  Under a numbering whose ids depend on the earlier groups' sizes the later
    groups' buckets would move.  Here their results and evidence are what they were, and the store grows by the new pairs' runs
    at most."""
    rows, segs = _library_of_four_groups(extra=1)
    _plant_extra(rows, segs, 12, A, 5)
    labels = LABELS12 + [A]
    pool = Videos(rows, even_timestamps(rows))
    live = Live(pool, labels, monkeypatch, min_s=20)
    live.add([0, 1, 2, 3, 4, 5, 6])
    live.add([7, 8, 9, 10, 11])
    before, before_evidence, slots_before = _as(live.index.results()), live.index.evidence(), live.index.store_sizes()[1]
    live.add([12])
    assert live.index.pairs_searched()[1] == 5
    after, after_evidence = _as(live.index.results()), live.index.evidence()
    others = [v for v in range(12) if labels[v] != A]
    assert [after[v] for v in others] == [before[v] for v in others]
    assert [after_evidence[v] for v in others] == [before_evidence[v] for v in others]
    group = [v for v in range(13) if labels[v] == A]
    runs = M.oracle_runs([[rows[v][0]] for v in group], 10, M.min_len_for(20), threads=8)
    pairs = [(i, j) for i in range(len(group)) for j in range(i + 1, len(group))]
    new_runs = sum(1 for r in runs if pairs[int(r["problem"])][1] == len(group) - 1)
    grown = live.index.store_sizes()[1] - slots_before
    assert 0 < grown <= new_runs, (grown, new_runs)


# ---- 3. a group of 258 among others ---------------------------------------------------------------------------------------------------
def test_a_group_of_258_crosses_the_256_slot_stage(monkeypatch):
    """best_match_kernel and match_evidence_kernel take a video's pair slots 256 at a time.  257 members of one group with two
    small groups interleaved, then the 258th alone: every member's candidate list changes, all 258 are recomputed."""
    labels = []
    for v in range(258):
        if v == 257:
            break
        labels.append(9)
        if v % 60 == 7:
            labels.append(0xFFFFFFFF)
        if v % 90 == 11:
            labels.append(3)
    labels.append(9)
    assert labels.count(9) == 258 and labels.count(0xFFFFFFFF) == 5 and labels.count(3) == 3 and labels[-1] == 9
    rng = np.random.default_rng(12)
    rows = random_rows(rng, [100 + int(x) for x in rng.integers(0, 31, len(labels))])
    seg9, seg5, seg3 = (_new(rng, k) for k in (40, 52, 46))
    for v, label in enumerate(labels):
        seg = seg9 if label == 9 else seg5 if label == 0xFFFFFFFF else seg3
        at = 3 + (v * 7) % 40
        flips = (np.uint32(1) << rng.integers(0, 32, len(seg)).astype(np.uint32)) * (rng.random(len(seg)) < 0.2)
        rows[v][0][at:at + len(seg)] = seg ^ (flips.astype(np.uint32) if v % 3 else np.uint32(0))   # a third of them exact copies
    pool = Videos(rows, even_timestamps(rows))
    live = Live(pool, labels, monkeypatch, min_s=5, evidence=False)
    n = len(labels)
    live.add(list(range(n - 1)))
    before = _as(live.index.results())
    live.add([n - 1])
    assert live.index.pairs_searched()[1] == 257
    got = _as(live.index.results())
    assert sum(1 for v in range(n) if labels[v] == 9 and got[v] is not None and got[v][0] is not None) >= 250
    assert [got[v] for v in range(n - 1) if labels[v] != 9] == [before[v] for v in range(n - 1) if labels[v] != 9]
    live.check_evidence()                 # 257 slots a video: the evidence kernel's second round of slots, against the host definition
    last = live.index.evidence()[n - 1].opening
    assert last is not None and not last.is_source and last.candidates > 1   # the last member: the destination of every one of its pairs


# ---- 4. two regions ---------------------------------------------------------------------------------------------------------------------
def test_two_regions_and_videos_without_ending_data(monkeypatch):
    """include_endings, rows of unequal lengths, every video its own timestamp step and origin.  A video without ending data
    fails the append when its group has another member (the index is as it was) and is accepted alone in its group."""
    labels = [1, 2, 1, 3, 2, 1, 2, 3, 1]
    rng = np.random.default_rng(14)
    rows = random_rows(rng, [380 + 17 * v for v in range(len(labels))], regions=2)
    for m in members_of(labels):
        for r in range(2):
            seg = _new(rng, 110 + 12 * r)
            for k, v in enumerate(m):
                flips = (np.uint32(1) << rng.integers(0, 32, len(seg)).astype(np.uint32)) * (rng.random(len(seg)) < 0.3)
                rows[v][r][10 + 11 * k + 5 * r: 10 + 11 * k + 5 * r + len(seg)] = seg ^ flips.astype(np.uint32)
    for r in range(2):
        cross = _new(rng, 200)
        rows[0][r][170:370] = cross
        rows[1][r][175:375] = cross
        rows[3][r][160:360] = cross
    ts = [[[2_000_000_000 + 1_000_003 * v + 5_000 * NS * r + i * (246_000_000 + 1_000 * v) for i in range(len(row))]
           for r, row in enumerate(video)] for v, video in enumerate(rows)]
    pool = Videos(rows, ts)
    # video 9: video 4's opening and no ending data at all
    opening = list(zip(rows[4][0].tolist(), ts[4][0]))
    pool.c.append(capi.FrameHashes.new(opening, [], HD))
    pool.o.append(O.FrameHashes(opening, [], HD, ""))
    pool.rows.append([rows[4][0], np.zeros(0, dtype=np.uint32)])
    live = Live(pool, labels + [2], monkeypatch, min_s=15, padding=0.5, evidence=False)   # (uneven timestamps: no run-length model)
    live.add([0, 1, 2, 3])
    live.add([4, 5, 6, 7, 8])
    want = live.expect()
    assert all(r is not None and r[0] is not None and r[1] is not None for r in want)
    before = live.state()
    with pytest.raises(capi.NeedleError, match="no ending hash data present"):
        live.index.add([pool.c[9]], groups=[2])                          # group 2 has three members
    assert live.state() == before
    live.pool_labels[9] = 4040                                            # alone in a group of its own: accepted, no result
    live.add([9])
    assert live.index.results()[9] is None and live.index.pairs_searched()[1] == 0
    with pytest.raises(capi.NeedleError, match="no ending hash data present"):
        live.index.replace([4], [pool.c[9]])                             # position 4 is of group 2
    live.check(0)


# ---- 5. remove and replace ------------------------------------------------------------------------------------------------------------
def test_remove_and_replace_inside_groups(monkeypatch):
    """Padding of 40 s, every group's segment beyond 100 s: a replacement whose segment ends at 33 s fails in best_match, after
    the rebuilt store was written, and leaves everything as it was."""
    rows, segs = _library_of_four_groups(at0=300, extra=3, kept=1000)
    _plant_extra(rows, segs, 12, B, 6)                                    # a replacement for a member of B
    rows[13][0][2:124] = segs[B][0]                                       # ... one that fails: its match ends before the padding
    _plant_extra(rows, segs, 14, C2, 4)                                   # a third member for C2
    labels = LABELS12 + [B, B, C2]
    pool = Videos(rows, even_timestamps(rows))
    live = Live(pool, labels, monkeypatch, min_s=20, padding=40.0)
    live.add(list(range(5)))
    live.add(list(range(5, 12)))
    assert all(r is not None and r[0] is not None for v, r in enumerate(_as(live.index.results())) if v != 6)
    live.remove([4])                     # a middle member of B: the ranks behind it drop
    live.remove([0])                     # the first video of the list: group numbers shift (B is group 0 now)
    assert live.labels[0] == B
    at = live.labels.index(B, 1)
    live.replace([at], [12])             # a member of B: its label is kept, only B's pairs are searched
    assert live.index.groups()[at] == B and live.index.pairs_searched()[1] == live.labels.count(B) - 1 == 2
    before = live.state()
    with pytest.raises(capi.NeedleError, match="overflow when subtracting durations"):
        live.index.replace([at], [pool.c[13]])
    assert live.state() == before
    with pytest.raises(capi.NeedleError) as e:
        live.index.remove([len(live.cur)])
    assert e.value.name == "InvalidArgument" and live.state() == before
    live.check(2)
    first_c2 = live.labels.index(C2)
    live.remove([first_c2])              # a group's last member but one: the remaining member has no result
    left = live.labels.index(C2)
    assert live.labels.count(C2) == 1 and live.index.results()[left] is None
    live.remove([left])                  # ... and the whole group
    assert C2 not in live.index.groups()
    live.remove([v for v, g in enumerate(live.labels) if g == A])   # a whole group at once
    live.add([14, 9])                    # C2 comes back as the last group: two arriving members, one pair
    assert live.index.pairs_searched()[1] == 1
    live.check_store()


# ---- 7. the host fallback ---------------------------------------------------------------------------------------------------------------
def test_host_fallback_on_a_grouped_append_and_replacement(monkeypatch):
    """Videos 0 and 2 (one group) hold one hash 40 times: ~39 runs in their pair's bucket, past what a lane orders.  With the
    large kernel switched off the bucket is the host's: on the append that brings video 2, and on the replacement of video 0."""
    labels = [3, 8, 3, 8, 3, 3]
    rng = np.random.default_rng(13)
    rows = random_rows(rng, [300] * 6)
    for k, v in enumerate((0, 2, 5)):
        rows[v][0][30 + 7 * k: 30 + 7 * k + 40] = np.uint32(0x0F1E2D3C)
    seg = _new(rng, 90)
    for v in range(6):
        rows[v][0][200:290] = seg                                         # an ordinary segment everybody shares, across groups too
    pool = Videos(rows, even_timestamps(rows))
    live = Live(pool, labels, monkeypatch, min_s=5, evidence=False)
    live.add([0, 1])
    assert live.fallbacks == 0
    monkeypatch.setenv("NEEDLE_HIP_EPILOGUE_NO_LARGE", "1")
    live.add([2, 3, 4])
    assert live.fallbacks == 1, "this append's entries came from the host"
    live.replace([0], [5])
    assert live.fallbacks == 1, "this replacement's entries came from the host"
    monkeypatch.delenv("NEEDLE_HIP_EPILOGUE_NO_LARGE")
    live.replace([0], [0])               # the large kernel under the grouped numbering: no fallback
    assert live.fallbacks == 0
    assert all(r is not None and r[0] is not None for r in _as(live.index.results()))


# ---- 8. refusals with a device ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_index_as_it_was(monkeypatch):
    rows, _ = _library_of_four_groups()
    pool = Videos(rows, even_timestamps(rows))
    live = Live(pool, LABELS12, monkeypatch, min_s=20, evidence=False)
    live.add(list(range(8)))
    plain = capi.Index(live.cmp)
    plain.add(pool.c[:8])
    before, plain_before = live.state(), (len(plain), _as(plain.results()), plain.pairs_searched())
    min_len = M.min_len_for(20)

    def refused(call, words):
        with pytest.raises(capi.NeedleError) as e:
            call()
        assert e.value.name == "InvalidArgument" and words in str(e.value), str(e.value)

    refused(lambda: live.index.add(pool.c[8:10]), "takes a label per video")
    refused(lambda: plain.add(pool.c[8:10], groups=[A, C2]), "not a grouped index")
    refused(lambda: plain.groups(), "not a grouped index")
    refused(lambda: live.index.crossmatcher(2, [700], [min_len]), "no streamed routes")
    refused(lambda: live.index.matcher(2), "no streamed routes")
    cross, lanes = plain.crossmatcher(2, [700], [min_len]), plain.matcher(2)   # (made from the plain twin: the kind of index is looked at first)
    refused(lambda: live.index.add_matched(cross, pool.c[8:10]), "no streamed routes")
    refused(lambda: live.index.add_streamed(lanes, None, pool.c[8:9]), "no streamed routes")
    assert live.state() == before
    assert (len(plain), _as(plain.results()), plain.pairs_searched()) == plain_before
    live.add([8, 9, 10, 11])             # and both go on working
    plain.add(pool.c[8:])
    assert _as(plain.results()) == _as(O.run_with_frame_hashes(live.ocmp, pool.o, threads=8))


# ---- 9. a plain index is untouched --------------------------------------------------------------------------------------------------------
def test_a_plain_append_launches_what_it_launched(monkeypatch):
    """The launches of one append on a plain index, before and after a grouped index has been used in the same process."""
    rows, _ = _library_of_four_groups()
    pool = Videos(rows, even_timestamps(rows))
    cmp, ocmp = pool.comparators(min_s=20)
    first, second = capi.Index(cmp), capi.Index(cmp)
    for ix in (first, second):
        ix.add(pool.c[:7])
    before = timed(lambda: first.add(pool.c[7:]))
    live = Live(pool, LABELS12, monkeypatch, min_s=20)
    live.add(list(range(7)))
    live.add(list(range(7, 12)))
    live.remove([2])
    after = timed(lambda: second.add(pool.c[7:]))
    print(before, after)
    assert before == after and before.get("index_best_match") == 1 and before.get("index_entries") == 1
    assert _as(first.results()) == _as(second.results()) == _as(O.run_with_frame_hashes(ocmp, pool.o, threads=8))
