"""-m gpu: the streaming comparator (needle_hip_matcher_*).  The checker is the oracle's table DP, used as
tests/test_gpu_scan_threshold.py uses it (timestamps = row index, min_opening_duration = min_len), and next to it
capi.hamming_runs on the same inputs; runs are compared as sorted tuples (src_end, dst_end, len, src_match_hash,
dst_match_hash) per source."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from needle_amd import capi, synth
from tests.test_gpu_scan_threshold import _dp_runs, _masks, _popcount

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M = 257                                 # the lane of tests 1, 2 and 4
SOURCE_LENS = (1, 2, 37, 300)
THRESHOLDS = (0, 10, 32)
MIN_LENS = (1, 8, 23)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


# ---- the planted table ----------------------------------------------------------------------------------------------------
class Planted:
    """Sources of 1, 2, 37 and 300 hashes and a lane of 257 on a random background.  Everything is planted on the source of 300
    (`big`); the source of 37 is its last 37 rows, so that the run that ends in big's last row ends in its last row too, and the
    source of 2 is its first two rows (row 1 is a cell, row 0 is not).  A structure is a stretch of rows a .. a + L - 1 and
    its own block of columns b .. b + L - 1 with every cell at distance exactly t, fenced by a cell at t + 1 at both ends."""

    def __init__(self, t, min_len, seed=1):
        rng = np.random.default_rng(seed * 7919 + t * 101 + min_len)
        n, T = SOURCE_LENS[-1], min(t, 32)
        fence = t + 1 if t + 1 <= 32 else None
        big = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        dst = rng.integers(0, 2 ** 32, M, dtype=np.uint64).astype(np.uint32)
        self.t, self.min_len, self.whole, self.cuts = t, min_len, [], set()
        L1 = min_len + 1

        def put(a, b, dists, name, before="fence", after="fence"):
            dists = np.asarray(dists, dtype=np.int64)
            L = len(dists)
            assert a >= 1 and a + L <= n and b >= 1 and b + L <= M, (name, a, b, L)
            rows, want = np.arange(a, a + L), dists.copy()
            if before == "match" or (before == "fence" and fence is not None):   # "match": a matching cell in row 0 or column 0
                rows, want = np.concatenate([[a - 1], rows]), np.concatenate([[T if before == "match" else fence], want])
            if after == "fence" and fence is not None and a + L < n and b + L < M:
                rows, want = np.concatenate([rows, [a + L]]), np.concatenate([want, [fence]])
            cols = rows - a + b
            dst[cols] = big[rows] ^ _masks(want, rng, int(rows[0]))
            assert _popcount(big[rows] ^ dst[cols]).tolist() == want.tolist(), name
            k = 0
            while k < L:                                                         # the stretches at <= t: what the oracle must list
                if dists[k] > t:
                    k += 1
                    continue
                e = k
                while e + 1 < L and dists[e + 1] <= t:
                    e += 1
                if e - k + 1 >= min_len:
                    self.whole.append((name, a + e, b + e, e - k + 1))
                k = e + 1
            return b + L + 2

        # a run from column 1 (column 0 holds a matching cell in front of it) and one from row 1 (row 0 likewise)
        b = put(40, 1, [T] * L1, "starts at j = 1", before="match")
        first_row_at = b + 1
        b = put(1, first_row_at, [T] * L1, "starts at i = 1", before="match")
        self.cuts.add(first_row_at + L1)                                         # ... whose last cell is a feed's last column
        # exactly min_len, its first cell the first column of a feed, and one cell short of min_len
        self.cuts.add(b + 1)
        b = put(70, b + 1, [T] * min_len, "exactly min_len")
        if min_len > 1:
            b = put(100, b + 1, [T] * (min_len - 1), "min_len - 1")
        # two runs with a single cell at t + 1 between them; the second one (columns s ..) crosses three feed boundaries
        broken = [T] * min_len + [min(t + 1, 32)] + [T] * (min_len + 3)
        s = b + 1 + min_len + 1
        self.cuts |= {b + 2, s + 1, s + 2, s + 3}
        b = put(130, b + 1, broken, "broken by t + 1")
        # a block of equal hashes, 12 rows x 10 columns, across a feed boundary
        h = np.uint32(rng.integers(0, 2 ** 32))
        big[200:212] = h
        dst[b:b + 10] = h
        self.cuts.add(b + 5)
        b += 12
        b = put(n - L1, b + 1, [T] * L1, "ends at i = n - 1")
        assert b + 1 <= M - L1, (b, min_len)
        put(230, M - L1, [T] * L1, "ends at j = m - 1")
        assert all(0 < c < M for c in self.cuts)
        lone = rng.integers(0, 2 ** 32, 1, dtype=np.uint64).astype(np.uint32)
        self.sources = [lone, big[:2].copy(), big[n - SOURCE_LENS[2]:].copy(), big]
        self.min_lens = [min_len] * len(self.sources)
        self.dst = dst
        assert tuple(len(s) for s in self.sources) == SOURCE_LENS

    _oracle = None

    def oracle(self):
        """{source: sorted runs} of the whole lane, computed once."""
        if self._oracle is None:
            self._oracle = {q: _dp_runs(s, self.dst, self.t, self.min_len) for q, s in enumerate(self.sources)}
            if self.t < 32:                                                      # what was planted is there
                for name, i, j, L in self.whole:
                    assert any(r[:3] == (i, j, L) for r in self._oracle[3]), (name, i, j, L)
            assert not self._oracle[0] and len(self._oracle[3]) >= 6
        return self._oracle


_TABLES = {}


def planted(t, min_len):
    if (t, min_len) not in _TABLES:
        _TABLES[(t, min_len)] = Planted(t, min_len)
    return _TABLES[(t, min_len)]


def by_source(runs):
    out = {}
    for x in runs:
        out.setdefault(int(x["problem"]), []).append((int(x["src_end"]), int(x["dst_end"]), int(x["len"]),
                                                      int(x["src_match_hash"]), int(x["dst_match_hash"])))
    return {k: sorted(v) for k, v in out.items()}


def nonempty(d):
    return {k: v for k, v in d.items() if v}


def one_shot(sources, min_lens, dst, t):
    """capi.hamming_runs over the same problems: {source: sorted runs}."""
    seqs = [*sources, dst]
    return by_source(capi.hamming_runs(seqs, [(q, len(sources), min_lens[q]) for q in range(len(sources))], t))


def stream(sources, min_lens, dst, t, sizes):
    """One lane fed in chunks of `sizes` (zeros are empty feeds), finished: ({source: sorted runs}, stats)."""
    m = capi.Matcher(sources, min_lens, 1, t)
    pos = 0
    for size in sizes:
        m.feed([dst[pos: pos + size]])
        pos += size
    assert pos == len(dst) and m.ready(0)[1:] == (len(dst), False)
    m.finish()
    assert m.ready(0)[1:] == (len(dst), True)
    return by_source(m.runs(0)), m.stats()


def sizes_from_cuts(cuts, total, rng=None):
    edges = [0, *sorted(cuts), total]
    sizes = [b - a for a, b in zip(edges, edges[1:])]
    if rng is not None:                                                          # empty feeds in between
        for at in sorted(rng.integers(0, len(sizes), 4).tolist(), reverse=True):
            sizes.insert(at, 0)
    return sizes


def cuttings(p):
    yield "one feed", [M]
    yield "one item per feed", [1] * M
    for seed in range(5):
        rng = np.random.default_rng(100 + seed)
        extra = set(rng.choice(np.arange(1, M), size=int(rng.integers(3, 40)), replace=False).tolist())
        yield f"random {seed}", sizes_from_cuts(p.cuts | extra, M, rng)
    yield "a first feed of one item", sizes_from_cuts(p.cuts | {1}, M)


# ---- 1. any cutting equals the one-shot and the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("min_len", MIN_LENS)
@pytest.mark.parametrize("t", THRESHOLDS)
def test_any_cutting_equals_the_one_shot_and_the_oracle(t, min_len):
    p = planted(t, min_len)
    want = nonempty(p.oracle())
    assert one_shot(p.sources, p.min_lens, p.dst, t) == want
    for name, sizes in cuttings(p):
        assert sum(sizes) == M, name
        got, _ = stream(p.sources, p.min_lens, p.dst, t, sizes)
        assert got == want, name


# ---- 2. reported when the rule says so ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_len", MIN_LENS)
@pytest.mark.parametrize("t", THRESHOLDS)
def test_runs_are_reported_when_the_rule_says_so(t, min_len):
    """After columns [0, J): exactly the runs with dst_end < J - 1, or in the source's last row with dst_end <= J - 1; `open`
    holds the others that touch column J - 1 and are already min_len long."""
    p = planted(t, min_len)
    m = capi.Matcher(p.sources, p.min_lens, 1, t)
    before = []
    for J in range(1, M + 1):
        m.feed([p.dst[J - 1: J]])
        count, fed, finished = m.ready(0)
        assert (fed, finished) == (J, False)
        raw = m.runs(0, 0, count)
        now = [tuple(int(v) for v in x) for x in raw]
        assert now[:len(before)] == before, J                                    # appended, never revised
        before = now
        prefix = {q: _dp_runs(s, p.dst[:J], t, min_len) for q, s in enumerate(p.sources)}
        closed = {q: [r for r in runs if r[1] < J - 1 or (r[0] == len(p.sources[q]) - 1 and r[1] <= J - 1)]
                  for q, runs in prefix.items()}
        assert by_source(raw) == nonempty(closed), J
        still = {q: [(r[0], r[1], r[2], 0, 0) for r in runs if r[1] == J - 1 and r[0] < len(p.sources[q]) - 1]
                 for q, runs in prefix.items()}
        opened = m.open(0)
        assert by_source(opened) == nonempty(still), J
        assert by_source(m.open(0)) == by_source(opened) and m.ready(0)[0] == count   # a function of the state alone
    m.finish()
    assert by_source(m.runs(0)) == nonempty(p.oracle())
    assert [tuple(int(v) for v in x) for x in m.runs(0)][:len(before)] == before
    assert len(m.open(0)) == 0


# ---- 3. lanes out of step ---------------------------------------------------------------------------------------------------
def test_lanes_out_of_step():
    rng = np.random.default_rng(5)
    t, sources = 10, [rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32) for n in (90, 2, 260)]
    min_lens = [4, 1, 6]

    def sequence(length, seed):
        r = np.random.default_rng(seed)
        d = r.integers(0, 2 ** 32, length, dtype=np.uint64).astype(np.uint32)
        for q, a, L in ((0, 20, 30), (2, 100, 45), (2, 1, 12)):                  # copies of source stretches with a few bits flipped
            if length > L + 2:
                b = int(r.integers(1, length - L))
                d[b:b + L] = sources[q][a:a + L] ^ _masks([3] * L, r, 0)
        return d
    lengths = (2, 57, 400, 129, 256)
    lanes = [sequence(n, 10 + k) for k, n in enumerate(lengths)]
    again = sequence(77, 99)                                                     # what lane 1 is reused for
    want = [nonempty({q: _dp_runs(s, d, t, min_lens[q]) for q, s in enumerate(sources)}) for d in [*lanes, again]]
    assert all(w == one_shot(sources, min_lens, d, t) for w, d in zip(want, [*lanes, again]))
    assert sum(len(v) for v in want[2].values()) >= 3 and want[5]

    m = capi.Matcher(sources, min_lens, 5, t)
    pos = [0] * 5
    step = 0
    while any(pos[k] < lengths[k] for k in range(5)):
        chunk = []
        for k in range(5):
            take = 0 if (step + k) % 3 == 0 else int(rng.integers(0, 70))          # some lanes get nothing
            chunk.append(lanes[k][pos[k]: pos[k] + take] if take else None)
            pos[k] = min(lengths[k], pos[k] + take)
        m.feed(chunk)
        step += 1
        if pos[1] == lengths[1] and not m.ready(1)[2]:                           # lane 1 finishes early, the others go on
            m.finish([1])
            assert by_source(m.runs(1)) == want[1]
        if m.ready(1)[2] and step % 2:
            with pytest.raises(capi.NeedleError) as e:                           # refused as a whole: no lane moves
                m.feed([lanes[0][:0], again[:5], None, None, None])
            assert e.value.code == capi.ERROR_NAMES.index("InvalidArgument")
    assert m.ready(1)[2] and [m.ready(k)[1] for k in range(5)] == list(lengths)
    m.reset([1])
    assert m.ready(1) == (0, 0, False)
    for a in range(0, len(again), 31):
        m.feed([None, again[a:a + 31], None, None, None])
    m.finish()
    for k in (0, 2, 3, 4):
        assert by_source(m.runs(k)) == want[k], k
    assert by_source(m.runs(1)) == want[5]
    # the errors that need an object
    invalid = capi.ERROR_NAMES.index("InvalidArgument")
    for call in (lambda: m.finish([5]), lambda: m.reset([5]), lambda: m.ready(5), lambda: m.runs(5), lambda: m.open(5),
                 lambda: m.runs(0, 0, m.ready(0)[0] + 1), lambda: m.feed([None, None, None, again, None]),
                 lambda: m.feed_from_feeder(capi.Feeder(4))):
        with pytest.raises(capi.NeedleError) as e:
            call()
        assert e.value.code == invalid


# ---- 4. every cell once, fixed launches ---------------------------------------------------------------------------------------
def test_every_cell_once_and_fixed_launches():
    p = planted(10, 8)
    _, (feeds, launches, cells, _) = stream(p.sources, p.min_lens, p.dst, 10, [1] * M)
    least = sum((n - 1) * (M - 1) for n in SOURCE_LENS)
    assert feeds == M and least <= cells <= least + sum(n * feeds for n in SOURCE_LENS)
    per_feed = launches // (feeds + 1)                                           # the finish is a round as well
    assert launches == per_feed * (feeds + 1)

    rng = np.random.default_rng(8)
    many = [rng.integers(0, 2 ** 32, int(n), dtype=np.uint64).astype(np.uint32) for n in rng.integers(2, 120, 40)]
    m = capi.Matcher(many, [3] * 40, 5, 10)
    chunk = rng.integers(0, 2 ** 32, 6, dtype=np.uint64).astype(np.uint32)
    state = []
    for k in range(30):
        was = m.stats()[1]
        m.feed([chunk if (k + lane) % 2 else None for lane in range(5)])         # only the lanes with data differ
        assert m.stats()[1] - was == per_feed, k
        state.append(m.stats()[3] - 4 * sum(m.ready(lane)[1] for lane in range(5)))
    assert state[9] == state[-1] and len(set(state)) == 1


# ---- 5. slab overflow ---------------------------------------------------------------------------------------------------------
_SLAB_CHILD = """
import json, sys
import numpy as np
from needle_amd import capi
from tests.test_gpu_matcher import by_source
src = np.full(64, 0x5A5A5A5A, dtype=np.uint32)
dst = np.full(64, 0x5A5A5A5A, dtype=np.uint32)
m = capi.Matcher([src], [8], 1, 10)
for a in range(0, 64, 16):
    m.feed([dst[a:a + 16]])
m.finish()
print(json.dumps({"runs": by_source(m.runs(0))[0], "stats": m.stats()}))
"""


def _slab_child(slab):
    env = {k: v for k, v in os.environ.items() if k != "NEEDLE_HIP_MATCHER_RUN_SLAB"}
    if slab:
        env["NEEDLE_HIP_MATCHER_RUN_SLAB"] = str(slab)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", _SLAB_CHILD], cwd=ROOT, env=env, stdout=subprocess.PIPE, text=True, timeout=120, check=True)
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_a_slab_too_small_loses_nothing():
    src = np.full(64, 0x5A5A5A5A, dtype=np.uint32)
    want = _dp_runs(src, src, 10, 8)
    assert len(want) > 100                                                       # every diagonal of 8 cells or more is a run
    small, roomy = _slab_child(4), _slab_child(0)
    assert [tuple(r) for r in small["runs"]] == want == [tuple(r) for r in roomy["runs"]]
    assert small["stats"][1] > roomy["stats"][1]                                 # the repeated rounds
    assert small["stats"][0] == roomy["stats"][0] == 4
    assert "NEEDLE_HIP_MATCHER_RUN_SLAB" not in os.environ


# ---- 6. from a feeder ---------------------------------------------------------------------------------------------------------
def _from_a_feeder():
    pcms = [synth.make_episode(k, 60.0, 20.0).pcm for k in range(3)]            # every episode holds the same 20 s intro
    lane = synth.make_episode(3, 90.0, 20.0).pcm                                 # ... in its first half
    sources = capi.fingerprint(pcms, 1, 2)
    want_items = capi.fingerprint([lane], 1, 2)[0]
    t, min_lens = 10, [40] * 3
    want = one_shot(sources, min_lens, want_items, t)
    assert sorted(want) == [0, 1, 2] and min(max(r[2] for r in runs) for runs in want.values()) >= 60   # 20 s: ~80 kept items
    f = capi.Feeder(1, 1, 11025, capi.SAMPLE_S16, 2)
    m = capi.Matcher(sources, min_lens, 1, t)
    early = 0
    for a in range(0, len(lane), 11025 // 2):
        f.feed([lane[a: a + 11025 // 2]])
        m.feed_from_feeder(f)
        assert m.ready(0)[1] == f.ready(0)[0] and not m.ready(0)[2]
        early = max(early, max((int(x["len"]) for x in m.runs(0)), default=0))
    assert early >= 60, "the shared segment's run is reported before the feeder is finished"
    f.finish()
    m.feed_from_feeder(f)
    assert m.ready(0)[1:] == (len(want_items), True)
    assert by_source(m.runs(0)) == want
    m.feed_from_feeder(f)                                                        # nothing new: nothing happens
    assert by_source(m.runs(0)) == want


def test_from_a_feeder():
    _from_a_feeder()


def test_from_a_feeder_f64(monkeypatch):
    monkeypatch.setenv("NEEDLE_HIP_STFT", "f64")
    _from_a_feeder()


# ---- 7. existing paths untouched ----------------------------------------------------------------------------------------------
def test_existing_paths_launch_no_matcher_kernel():
    eps = synth.make_library(3, 60.0, 15.0)
    pcms = [e.pcm for e in eps]
    p = planted(10, 8)
    names = ("matcher_land", "matcher_strip", "matcher_simhash")
    capi.set_kernel_timing("all,sum")
    try:
        one_shot(p.sources, p.min_lens, p.dst, 10)
        lib = capi.Library(len(pcms))
        lib.set_pcm(pcms, [len(x) for x in pcms])
        cmp = capi.Comparator([f"ep{k}.wav" for k in range(len(pcms))], min_opening_duration=10)
        lib.job_begin(cmp, 0)
        lib.job_end(cmp, 0)
        capi.synchronize()
        assert capi.last_kernel_ms("simhash_runs") >= 0 or capi.last_kernel_ms("hamming_runs") >= 0
        assert all(capi.last_kernel_ms(k) < 0 for k in names), "no matcher kernel in a one-shot scan or a library job"
        stream(p.sources, p.min_lens, p.dst, 10, [M])
        capi.synchronize()
        assert all(capi.last_kernel_ms(k) >= 0 for k in names)
    finally:
        capi.set_kernel_timing(None)


# ---- the paths the small tables do not take ---------------------------------------------------------------------------------
def test_a_feed_wider_than_a_strip_and_a_source_of_65536_rows():
    """A feed of more than 512 items is cut into strips (runs planted across the strip boundaries at columns 512 and 1024, and
    diagonals that enter through row 1 in every workgroup of such a strip); a source of 65 536 hashes or more switches the
    carried run lengths from 16 to 32 bits."""
    rng = np.random.default_rng(21)
    src = rng.integers(0, 2 ** 32, 700, dtype=np.uint64).astype(np.uint32)
    dst = rng.integers(0, 2 ** 32, 1300, dtype=np.uint64).astype(np.uint32)
    copies = ((1, 300, 600), (50, 950, 30), (300, 1000, 40), (640, 1, 59), (2, 1240, 60))
    for a, b, L in copies:
        dst[b:b + L] = src[a:a + L] ^ _masks([2] * L, rng, 0)
    want = nonempty({0: _dp_runs(src, dst, 9, 12)})
    ends = {r[:2]: r[2] for r in want[0]}                                         # (the background may lengthen a copy)
    assert all(ends.get((a + L - 1, b + L - 1), 0) >= L for a, b, L in copies)
    assert one_shot([src], [12], dst, 9) == want
    for sizes in ([1300], [700, 600], [3, 1297]):
        got, stats = stream([src], [12], dst, 9, sizes)
        assert got == want, sizes
        assert stats[1] == 3 * (sum(-(-s // 512) for s in sizes) + 1), sizes

    long_src = rng.integers(0, 2 ** 32, 65540, dtype=np.uint64).astype(np.uint32)
    short = rng.integers(0, 2 ** 32, 48, dtype=np.uint64).astype(np.uint32)
    short[5:45] = long_src[65500:65540] ^ _masks([1] * 40, rng, 0)                # a run into the last row, beyond row 65 535
    want = nonempty({0: _dp_runs(long_src, short, 9, 5)})
    assert any(r[:2] == (65539, 44) and r[2] >= 40 for r in want[0])
    assert one_shot([long_src], [5], short, 9) == want
    got, _ = stream([long_src], [5], short, 9, [20, 1, 27])
    assert got == want
