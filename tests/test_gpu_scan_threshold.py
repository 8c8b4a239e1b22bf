"""-m gpu: every scan form at the exact edge of the Hamming threshold.  A cell matches when popcount(src ^ dst) <= t
(comparator.rs:178-183), and three parts of the scan encode t in arithmetic rather than compare with it: the matrix-pipe
form's accumulator preset 63 - 4 t (its sign bit: d + d' <= 2 t over two head rows, scan_mfma_kernel.h), the bias 31 - t of
the vector and matrix-pipe exact tests (bit 5 of popcount + bias: a cell that does NOT match, search.hip), and the host's
routing (search.hip scan_switches / scan_plan.h build_plan: the matrix pipe up to t = 15, the band or generic kernel from t = 32).  An
off-by-one in any of them shows only on cells at distance exactly t or t + 1, which random hashes with single-bit noise never
line up into runs.  So the tables here are planted cell by cell at EXACT distances -- runs of cells at t, the same broken by
single cells at t + 1 on every kind of row an aligned window has, head-row pairs whose sum passes the matrix pipe's filter
while one of them is over t -- and every form's complete run list is compared with the oracle's table DP."""
import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests.test_gpu_parity import search_mode  # noqa: F401  (the fixture: every scan form on the same inputs)

pytestmark = pytest.mark.gpu
NS = O.NS

W = 8                                   # rows of an aligned window (search.hip kSampleW)
PROBES = 4                              # probe rows on either side of a window (scan_mfma_kernel.h kM2Probe)
ANCHORS = (0, 31, 15, 16)               # bit positions every mask set takes in turn: both ends of the word and the 15 | 16 seam
THRESHOLDS = (0, 1, 2, 5, 9, 10, 11, 14, 15, 16, 17, 23, 30, 31, 32)
MIN_LENS = (23, 41, 82, 21, 8)          # aligned-window kernels, then the band kernel's and the generic kernel's


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _popcount(x):
    return np.bitwise_count(np.asarray(x, dtype=np.uint32)).astype(np.int64)


def _masks(dists, rng, first_row):
    """One u32 per row with exactly dists[k] distinct set bits.  Row k's set starts with ANCHORS[(first_row + k) % 4] and the
    rest are drawn at random, so bit 0, bit 31 and both sides of the 15 | 16 seam (one FP4 nibble per hash bit in the matrix
    pipe's image) carry a flipped bit on every fourth row."""
    out = np.zeros(len(dists), dtype=np.uint32)
    for k, d in enumerate(dists):
        if d == 0:
            continue
        anchor = ANCHORS[(first_row + k) % len(ANCHORS)]
        others = rng.permutation([b for b in range(32) if b != anchor])[: d - 1]
        out[k] = np.uint32(sum(1 << int(b) for b in [anchor, *others]))
    return out


def _dp_runs(src, dst, thr, min_len):
    """The oracle's table DP (comparator.rs:175-247) with timestamps = row index, so that its duration test keeps exactly the
    runs of min_len cells or more (ts[end] - ts[end - len] = len) -- what _oracle_runs in test_gpu_parity filters in Python,
    filtered in C: a table of 4 M cells at t = 15 has half a million shorter runs."""
    cmp = O.Comparator(hash_match_threshold=thr, min_opening_duration=min_len)
    ents = O.longest_common_hash_match(cmp, [(int(h), i) for i, h in enumerate(src)],
                                       [(int(h), i) for i, h in enumerate(dst)], 0, 0)
    return sorted((e["src_end_idx"], e["dst_end_idx"], e["score"], e["src_match_hash"], e["dst_match_hash"]) for e in ents)


def _gpu_runs(seqs, problems, thr):
    r = capi.hamming_runs(seqs, problems, thr)
    out = {}
    for x in r:
        out.setdefault(int(x["problem"]), []).append((int(x["src_end"]), int(x["dst_end"]), int(x["len"]),
                                                      int(x["src_match_hash"]), int(x["dst_match_hash"])))
    return {k: sorted(v) for k, v in out.items()}


def _probe_offset(s, min_len):
    """scan_mfma_kernel.h m2_probe_offset (C division: truncated toward zero)."""
    reach = (min_len - W + 1) // 2
    i = -1 - s if s < 0 else s - W
    q = i * (reach - 1)
    dist = 1 + (abs(q) // (PROBES - 1)) * (1 if q >= 0 else -1)
    return -dist if s < 0 else W - 1 + dist


def _expected_form(mode, t, min_len):
    """needle_hip_scan_last_launch's form: 1 generic, 2 band, 3 sampled (vector), 4 sampled on the matrix pipe."""
    if mode == "generic" or min_len < 21:
        return 1
    if mode == "band" or t >= 32 or min_len < 2 * W - 1 + 8:
        return 2
    return 4 if mode == "sampled-mfma" and t <= 15 else 3


class _Table:
    """A random source x destination table with structures planted on their own diagonals.  A structure is a stretch of source
    rows a .. a + L - 1 and its own block of destination columns b .. b + L - 1 (dst[b + k] = src[a + k] ^ mask of dists[k] bits),
    fenced by a cell at t + 1 on both ends so that the background cannot lengthen it.  Structures share source rows, never
    destination columns: the source rows can sit wherever the window geometry wants them."""

    def __init__(self, t, n, rng):
        self.t, self.n, self.rng = t, n, rng
        self.plan = []                   # (a, dists, b or None for "next free block", name)

    def add(self, a, dists, name, b=None):
        assert 1 <= a and a + len(dists) <= self.n, (name, a, len(dists), self.n)
        self.plan.append((a, np.asarray(dists, dtype=np.int64), b, name))

    def build(self, margin=40):
        t, rng = self.t, self.rng
        fence = t + 1 if t + 1 <= 32 else None
        first = [p for p in self.plan if p[2] == 1]
        last = [p for p in self.plan if p[2] == "end"]
        middle = [p for p in self.plan if p[2] is None]
        need = sum(len(p[1]) + 2 + 3 for p in self.plan) + margin
        m = need
        self.m = m
        src = rng.integers(0, 2 ** 32, self.n, dtype=np.uint64).astype(np.uint32)
        dst = rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32)
        placed, b = [], 1
        for a, dists, fixed, name in first + middle + last:
            L = len(dists)
            if fixed == "end":
                b = m - L
            rows = np.arange(a, a + L)
            want = dists.copy()
            if fence is not None and a - 1 >= 0 and b - 1 >= 0:      # fences (row or column 0: never a cell of a run anyway)
                rows, want = np.concatenate([[a - 1], rows]), np.concatenate([[fence], want])
            if fence is not None and a + L < self.n and b + L < m:
                rows, want = np.concatenate([rows, [a + L]]), np.concatenate([want, [fence]])
            cols = rows - a + b
            dst[cols] = src[rows] ^ _masks(want, rng, int(rows[0]))
            placed.append((a, b, dists, name, rows, cols, want))
            b += L + 2 + int(rng.integers(1, 4))
        # what was planted is what was meant: every planted cell's distance, and no two structures on one column
        allcols = np.concatenate([p[5] for p in placed])
        assert len(np.unique(allcols)) == len(allcols) and allcols.min() >= 0 and allcols.max() < m
        for a, b, dists, name, rows, cols, want in placed:
            assert _popcount(src[rows] ^ dst[cols]).tolist() == want.tolist(), name
        self.src, self.dst, self.placed = src, dst, placed
        return src, dst


def _whole_runs(placed, t):
    """(src_end, dst_end, len) of every planted stretch of cells at distance <= t that its fences (or the table's edges) end."""
    out = []
    for a, b, dists, name, rows, cols, want in placed:
        k = 0
        while k < len(dists):
            if dists[k] > t:
                k += 1
                continue
            e = k
            while e + 1 < len(dists) and dists[e + 1] <= t:
                e += 1
            out.append((name, a + e, b + e, e - k + 1))
            k = e + 1
    return out


def _plant(t, min_len, seed):
    """The planted table for (t, min_len): see test_every_form_at_the_threshold_edge."""
    rng = np.random.default_rng(seed * 1_000_003 + t * 101 + min_len)
    P = min_len - W + 1

    def window_at_or_after(row):                                  # aligned windows start at rows 1 + k P
        return 1 + max(0, -(-(row - 1) // P)) * P
    T, F = min(t, 32), t + 1              # (t = 32: every cell matches; runs planted at 32 still differ from t = 31's)
    chain = None
    if F <= 32:
        # (b) one long copy of (a) broken by single cells at t + 1, each on another kind of row of an aligned window: head rows
        # 0, 2, 4, 7 (the FP4 products' pairs 0 | 2 and 4 | 7; the vector kernel's first three tests are rows 0, 4, 7), rows no
        # head test reads, the farthest and nearest probes on both sides, the middle of the gap -- and (c) head-row pairs whose
        # SUM passes the matrix pipe's filter, d + d' = (t + 1) + (t - 1) = 2 t, while the t + 1 row must end the run.
        # Between two breaks at least min_len // 2 rows: whatever a break separates would be a run of min_len or more if the
        # break were taken for a match.
        gap_mid = W + max(0, (P - W) // 2)
        breaks = [(0, None), (2, None), (4, None), (7, None), (1, None), (3, None), (6, None),
                  (_probe_offset(W + PROBES - 1, min_len), None), (_probe_offset(-PROBES, min_len), None),
                  (_probe_offset(W, min_len), None), (_probe_offset(-1, min_len), None), (gap_mid, None)]
        if t >= 1:
            breaks += [(2, 0), (7, 4), (0, 2)]
        stretch = [min_len // 2, (min_len + 1) // 2 + 1, min_len // 2 + 2, min_len + 2]
        start = window_at_or_after(20) + 2
        rows = {}
        prev = start - 1
        for k, (off, partner) in enumerate(breaks):
            target = prev + 1 + stretch[k % len(stretch)]
            x = target + (1 + off - target) % P                   # the first row >= target at offset `off` of its window
            rows[x] = F
            if partner is not None:
                rows[x - off + partner] = t - 1
            prev = x
        end = prev + min_len + 3
        chain = (start, [rows.get(r, T) for r in range(start, end + 1)])
    n = 1500 if t <= 16 else 700                                  # (from t = 17 on random cells match 70 - 100 % of the time)
    if chain is not None:
        n = max(n, chain[0] + len(chain[1]) + 2 * min_len + 10)
    tab = _Table(t, n, rng)
    # (a) runs whose every cell is at exactly t: one starting mid-gap, one starting on a window's first row
    tab.add(window_at_or_after(40) + 3, [T] * (3 * min_len + 5), "a: mid-gap")
    tab.add(window_at_or_after(300), [T] * (3 * min_len), "a: on a window")
    # (d) runs that touch row 1, column 1, the last row and the last column
    tab.add(1, [T] * (2 * min_len + 1), "d: row 1")
    tab.add(window_at_or_after(200) + 5, [T] * (2 * min_len + 3), "d: column 1", b=1)
    tab.add(n - (2 * min_len + 2), [T] * (2 * min_len + 2), "d: last row")
    tab.add(window_at_or_after(500) + 1, [T] * (2 * min_len), "d: last column", b="end")
    if chain is not None:
        tab.add(chain[0], chain[1], "b: breaks")
        # stretches of exactly min_len and min_len - 1 rows between cells at t + 1, the first starting on a window's first row,
        # and a copy of (a) whose first and last rows are at t + 1 (its run starts on a window's first row)
        w = window_at_or_after(150)
        ex = [T] * min_len + [F] + [T] * (min_len - 1) + [F] + [T] * min_len + [F] + [T] * (min_len - 1)
        tab.add(w, ex, "b: min_len and min_len - 1")
        w = window_at_or_after(260)
        tab.add(w - 1, [F] + [T] * (2 * min_len) + [F], "b: first and last row")
    src, dst = tab.build()
    return src, dst, tab.placed


_CASES = {}


def _case(t, min_len, seed=0):
    """Planted table, the DP's run list, and the proof that the boundary decides something -- once per (t, min_len, seed)."""
    key = (t, min_len, seed)
    if key not in _CASES:
        src, dst, placed = _plant(t, min_len, seed)
        want = _dp_runs(src, dst, t, min_len)
        ends = {(r[0], r[1], r[2]) for r in want}
        for name, i, j, L in _whole_runs(placed, t) if t < 32 else []:
            if L >= min_len and name.startswith(("a:", "d:")):
                assert (i, j, L) in ends, (name, t, min_len)
        if t < 32:                                                 # (from 32 on every cell matches: t + 1 changes nothing)
            assert _dp_runs(src, dst, t + 1, min_len) != want, ("t + 1 decides nothing", t, min_len)
        if t > 0:
            assert _dp_runs(src, dst, t - 1, min_len) != want, ("t - 1 decides nothing", t, min_len)
        _CASES[key] = (src, dst, placed, want)
    return _CASES[key]


@pytest.mark.parametrize("min_len", MIN_LENS)
@pytest.mark.parametrize("t", THRESHOLDS)
def test_every_form_at_the_threshold_edge(t, min_len, search_mode):  # noqa: F811
    """One table per (t, min_len), 1500 - 1600 source rows (700 from t = 17 on, where random cells match 70 - 100 % of the time,
    unless min_len 82's breaks need more):
    (a) runs of >= 3 min_len cells all at distance exactly t; (b) copies broken by single cells at t + 1 on head rows, rows no
    head test reads, probe rows, the gap, a run's first and last row, leaving stretches of exactly min_len and min_len - 1; (c)
    head-row pairs at t - 1 and t + 1; (d) runs on row 1, column 1, the last row and the last column.  Complete run lists
    against the table DP, and which form ran."""
    src, dst, placed, want = _case(t, min_len)
    got = _gpu_runs([src, dst], [(0, 1, min_len)], t).get(0, [])
    assert got == want, (search_mode, t, min_len, sorted(set(got) ^ set(want))[:8])
    assert capi.scan_last_launch()[0] == _expected_form(search_mode, t, min_len), (search_mode, t, min_len)
    assert len(want) >= 3


@pytest.mark.parametrize("waves,splits", [(4, 1), (4, 3), (8, 1), (8, 3), (16, 1), (16, 3)])
@pytest.mark.parametrize("t", [0, 15])
def test_matrix_pipe_presets_at_their_extremes_in_its_shapes(t, waves, splits, monkeypatch):
    """The matrix-pipe form at t = 0 (accumulator preset 63) and t = 15 (preset 3) in its workgroup shapes
    (NEEDLE_HIP_MFMA_WAVES) and workgroups per group (NEEDLE_HIP_MFMA_SPLITS), on the planted tables above with four sources
    per destination: the table's source and three copies shifted by 5, 17 and 40 rows, so that every planted row meets the
    aligned windows at another offset.  Complete run lists against the DP."""
    monkeypatch.setenv("NEEDLE_HIP_SCAN_MFMA", "1")
    monkeypatch.setenv("NEEDLE_HIP_MFMA_WAVES", str(waves))
    monkeypatch.setenv("NEEDLE_HIP_MFMA_SPLITS", str(splits))
    for min_len in (23, 41, 82):
        src, dst, placed, _ = _case(t, min_len)
        rng = np.random.default_rng(min_len)
        srcs = [src] + [np.concatenate([rng.integers(0, 2 ** 32, s, dtype=np.uint64).astype(np.uint32), src[: len(src) - s]])
                        for s in (5, 17, 40)]
        seqs = srcs + [dst]
        problems = [(k, len(srcs), min_len) for k in range(len(srcs))]
        got = _gpu_runs(seqs, problems, t)
        assert capi.scan_last_launch()[0] == 4
        for p, s in enumerate((0, 5, 17, 40)):
            key = ("shifted", t, min_len, s)
            if key not in _CASES:
                _CASES[key] = _dp_runs(srcs[p], dst, t, min_len)
            want = _CASES[key]
            assert got.get(p, []) == want, (t, min_len, s, waves, splits)
            ends = {(r[0], r[1], r[2]) for r in want}
            for name, i, j, L in _whole_runs(placed, t):
                if L >= min_len and name.startswith("a:"):
                    assert (i + s, j, L) in ends, (name, t, min_len, s)


def _min_len_for(ts, min_duration_ns):
    """needle_core.h min_run_length: the smallest L for which some ts[i] - ts[i - L] reaches the minimum duration."""
    ts = np.asarray(ts, dtype=np.int64)
    for L in range(1, len(ts)):
        if (ts[L:] - ts[:-L]).max() >= min_duration_ns:
            return L
    return 0


def test_library_job_takes_the_matrix_pipe_by_itself_at_the_threshold_edge(monkeypatch):
    """65 videos (2080 pairs: the scan takes the matrix-pipe form by itself) whose hash rows are written straight into the
    library's arena: a segment carried by video 0 and, at distance exactly t on every row, by twelve others; a second one whose
    copies are broken by single cells at t + 1; each fenced by cells at t + 1.  Jobs at t = 3 and 15 (matrix pipe) and 16 (the
    vector form): the job's results -- through the device epilogue -- and its complete run list against the oracle on the same
    rows."""
    monkeypatch.delenv("NEEDLE_HIP_SCAN_MFMA", raising=False)
    monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", "1")
    n, seconds, min_s = 65, 120.0, 10
    lens = [int(round(seconds * synth.RATE))] * n
    lib = capi.Library(n, opening_search_percentage=1.0)
    zeros = np.zeros(lens[0], dtype=np.int16)
    lib.stream_pcm([zeros] * n, lens)                              # geometry only: the rows are overwritten below
    f0 = lib.frame_hashes(0)
    kept = len(f0.opening_data()[0])
    ts = f0.opening_data()[1]
    min_len = _min_len_for(ts, min_s * NS)
    assert kept > 4 * min_len and min_len >= 2 * W - 1 + W
    d_arena, stride = lib.hash_arena()
    assert lib.rows_per_video() == 1
    hd = O.duration_from_secs_f32(0.3)
    for t, form in ((3, 4), (15, 4), (16, 3)):
        rng = np.random.default_rng(500 + t)
        rows = [rng.integers(0, 2 ** 32, kept, dtype=np.uint64).astype(np.uint32) for _ in range(n)]
        L = 3 * min_len
        seg_a, seg_b = (rng.integers(0, 2 ** 32, L + 2, dtype=np.uint64).astype(np.uint32) for _ in range(2))
        whole = []
        for v in range(0, 13):                                    # seg_a: video 0 as is, videos 1 .. 12 at exactly t
            at = 5 + 23 * (v % 7)
            dists = [0] * (L + 2) if v == 0 else [t + 1] + [t] * L + [t + 1]
            rows[v][at:at + L + 2] = seg_a ^ _masks(dists, rng, at)
            if v > 0:
                whole.append((v, at))
        brk = [t + 1] + [t] * L + [t + 1]
        for r in (min_len // 2, min_len + 4, 2 * min_len + 1):    # ... seg_b: broken three times
            brk[1 + r] = t + 1
        for v in range(20, 31):
            at = 9 + 17 * (v % 9)
            dists = [0] * (L + 2) if v == 20 else brk
            rows[v][at:at + L + 2] = seg_b ^ _masks(dists, rng, at)
        for v in range(1, 13):                                    # what was planted: exactly t against video 0
            a0, av = 5, 5 + 23 * (v % 7)
            d = _popcount(rows[0][a0:a0 + L + 2] ^ rows[v][av:av + L + 2])
            assert d.tolist() == [t + 1] + [t] * L + [t + 1], v
        for v in range(n):
            h = np.ascontiguousarray(rows[v])
            capi.check(capi.lib().needle_hip_memcpy_h2d(d_arena + 4 * v * stride, h.ctypes.data, h.nbytes))
        cmp = capi.Comparator([f"v{v}.wav" for v in range(n)], min_opening_duration=min_s, hash_match_threshold=t)
        slot = t % 2
        lib.job_begin(cmp, slot)
        res, found = lib.job_end(cmp, slot)
        jf = lib.job_form(slot)
        assert jf["scan_form"] == form and jf["device_epilogue"], (t, jf)
        runs = lib.job_runs(slot)
        assert len(runs) == found
        got = sorted(zip(*(runs[f].tolist() for f in ("problem", "src_end", "dst_end", "len", "src_match_hash", "dst_match_hash"))))
        total, ref = O.diagonal_runs_all_pairs(rows, t, min_len, threads=8, capacity=max(4 * found, 1 << 16))
        assert total == found, (t, total, found)
        pi, pj = np.triu_indices(n, 1)
        want = []
        for p, i_end, j_end, ln in ref.tolist():
            i, j = pi[p], pj[p]
            want.append((p, i_end, j_end, ln, O.simhash32(rows[i][i_end - ln:i_end + 1].tolist()),
                         O.simhash32(rows[j][j_end - ln:j_end + 1].tolist())))
        assert got == sorted(want), t
        pair = {(int(a), int(b)): p for p, (a, b) in enumerate(zip(pi, pj))}
        ends = {(r[0], r[1], r[2], r[3]) for r in got}
        for v, at in whole:                                       # every exact-t copy is a run of its own, fences and all
            assert (pair[(0, v)], 5 + L, at + L, L) in ends, (t, v)
        fhs = [O.FrameHashes(list(zip(rows[v].tolist(), ts.tolist())), [], hd, "") for v in range(n)]
        ref_res = O.run_with_frame_hashes(O.Comparator(hash_match_threshold=t, min_opening_duration=min_s * NS), fhs, threads=8)
        assert [None if r is None else (r.opening, r.ending) for r in res] == \
               [None if r is None else (r.opening, r.ending) for r in ref_res], t
        assert sum(1 for r in res if r is not None and r.opening is not None) >= 13
