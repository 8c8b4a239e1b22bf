"""-m gpu: removal and replacement in the incremental index (needle_hip_index_remove / _replace / _store_sizes) against the
oracle.  After every operation the index's results must equal, to the nanosecond, oracle.run_with_frame_hashes over the
CURRENT list (and capi.Comparator.run_with_frame_hashes over it), pairs_searched must follow the header's rules, and the
rebuilt store must hold no dead entry slot, exactly the current rows' hashes and at most as many timestamps.  What can go
wrong is the renumbering (pair ids, roles, the lower candidate index winning a tie), which videos are recomputed, the
timestamp rows shared with video 0, and what a failed operation leaves behind."""
import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests.test_gpu_index import HD, Corpus, _as, _planted, _segments
from tests.test_gpu_parity import search_mode  # noqa: F401  (the fixture: every scan form)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


class Live:
    """An index and the list it stands for: every operation is applied to both, then checked."""

    def __init__(self, pool, endings=None):
        self.pool = pool                       # a Corpus holding every video the test may use
        self.index = capi.Index(pool.comparator())
        self.cur = []                          # indices into the pool, in the index's order
        self.endings = pool.cfg["endings"] if endings is None else endings

    def rows(self):
        return sum(len(self.pool.o[p].opening) + (len(self.pool.o[p].ending) if self.endings else 0) for p in self.cur)

    def check(self, last):
        n = len(self.cur)
        assert len(self.index) == n
        view = Corpus(**self.pool.cfg)
        view.c = [self.pool.c[p] for p in self.cur]
        view.o = [self.pool.o[p] for p in self.cur]
        want = view.expect(n) if n else []
        assert _as(self.index.results()) == want, f"list {self.cur}"
        total, got_last = self.index.pairs_searched()
        assert got_last == last, (got_last, last)
        assert total == self.total
        held, slots, hashes, ts = self.index.store_sizes()
        assert held == slots, "dead entry slots after an edit"
        assert hashes == self.rows()
        assert ts <= hashes

    def add(self, pool_ids):
        n0, k = len(self.cur), len(pool_ids)
        self.index.add([self.pool.c[p] for p in pool_ids])
        self.cur += list(pool_ids)
        n = len(self.cur)
        last = n * (n - 1) // 2 - n0 * (n0 - 1) // 2
        self.total = getattr(self, "total", 0) + last
        total, got_last = self.index.pairs_searched()
        assert (total, got_last) == (self.total, last)
        assert _as(self.index.results()) == (self._expect() if n else [])

    def _expect(self):
        view = Corpus(**self.pool.cfg)
        view.c = [self.pool.c[p] for p in self.cur]
        view.o = [self.pool.o[p] for p in self.cur]
        return view.expect(len(self.cur))

    def remove(self, positions):
        self.index.remove(positions)
        self.cur = [p for q, p in enumerate(self.cur) if q not in set(positions)]
        self.check(0)

    def replace(self, positions, pool_ids):
        self.index.replace(positions, [self.pool.c[p] for p in pool_ids])
        for q, p in zip(positions, pool_ids):
            self.cur[q] = p
        n, k = len(self.cur), len(positions)
        last = k * (n - k) + k * (k - 1) // 2   # every pair with a replaced video (every row here can hold a run)
        self.total += last
        self.check(last)

    def state(self):
        return (len(self.index), _as(self.index.results()), self.index.pairs_searched(), self.index.store_sizes())


def _pool(seed, n, kept=600, endings=False, exact=False, min_s=10, padding=0.0, ts_shift=()):
    """Planted rows; the videos in ts_shift get timestamps of their own (not video 0's: a separate timestamp row)."""
    rng = np.random.default_rng(seed)
    pool = Corpus(endings=endings, min_s=min_s, padding=padding)
    for v, regions in enumerate(_planted(rng, n, kept, _segments(rng), endings=endings, exact=exact)):
        ts0 = 2_600_000_000 + (37_000_000 if v in ts_shift else 0)
        pool.add_rows(regions[0], regions[1] if endings else (), ts0=ts0)
    return pool


@pytest.mark.parametrize("endings", [False, True])
def test_remove_first_middle_last_several_down_to_none_then_add(endings):
    pool = _pool(31, 16, endings=endings, ts_shift=(0, 1))
    live = Live(pool)
    live.add(list(range(12)))
    live.remove([0])                 # video 0 had timestamps of its own, video 1 (now 0) too; the rest shared 0's
    live.remove([5])
    live.remove([len(live.cur) - 1])
    live.remove([6, 1, 3])
    live.remove(list(range(1, len(live.cur))))   # down to one video
    assert len(live.cur) == 1
    live.remove([0])                 # ... and to none
    assert live.index.store_sizes() == (0, 0, 0, 0) and live.index.results() == []
    live.add([12, 13])
    live.add([14, 15, 2])
    live.remove([1])
    live.add([0])


@pytest.mark.parametrize("endings,padding", [(False, 0.0), (True, 0.25)])
def test_replace_first_last_and_adjacent(endings, padding):
    pool = _pool(37, 16, endings=endings, min_s=15 if endings else 10, padding=padding, ts_shift=(10, 11))
    live = Live(pool)
    live.add(list(range(10)))
    live.replace([0], [10])          # position 0: the others still read the old video 0's timestamps
    live.add([12])                   # compares its timestamps with the NEW video 0's
    live.replace([len(live.cur) - 1], [13])
    live.replace([4, 5], [14, 15])
    live.replace([0], [11])
    live.remove([0])
    live.replace([2, 0], [10, 1])    # positions in any order


def test_ties_between_identical_episodes_after_renumbering():
    """Bit-identical episodes: the candidate index decides a tie, and removal renumbers the candidates."""
    rng = np.random.default_rng(7)
    pool = Corpus(min_s=10)
    base = rng.integers(0, 2 ** 32, 600, dtype=np.uint64).astype(np.uint32)
    for v in range(9):
        h = base.copy() if v % 3 else rng.integers(0, 2 ** 32, 600, dtype=np.uint64).astype(np.uint32)
        h[50:170] = base[50:170]
        pool.add_rows(h)
    for (op,) in _planted(rng, 6, 600, _segments(rng), exact=True):
        pool.add_rows(op)
    live = Live(pool)
    live.add(list(range(13)))
    live.remove([1])
    live.remove([0, 4])
    live.replace([2], [13])
    live.replace([0, 1], [14, 1])
    live.remove([len(live.cur) - 1, 3])


def test_hostile_corpus_large_buckets_and_listed_host_fallback(monkeypatch):
    """Silence against silence: a replacement's large buckets go to the workgroup kernel; with that kernel switched off
    (NEEDLE_HIP_EPILOGUE_NO_LARGE) the listed pairs' entries come from the host form."""
    n, samples = 12, int(8 * 60 * 11025)
    gen = synth.DeviceLibrary(n, samples, 45.0, hostile=True)
    lib = capi.Library(n, opening_search_percentage=1.0)
    lib.set_pcm_device(gen.pointers(), [samples] * n)
    lib.analyze()
    pool = Corpus(min_s=20)
    for v in range(n):
        pool.add_capi(lib.frame_hashes(v))
    gen.free()
    live = Live(pool)
    live.add(list(range(9)))
    live.replace([0], [9])
    live.remove([3])
    before = capi.epilogue_host_fallbacks()
    monkeypatch.setenv("NEEDLE_HIP_EPILOGUE_NO_LARGE", "1")
    live.replace([1, 6], [10, 11])
    assert capi.epilogue_host_fallbacks() > before, "the replacement's silent pairs fell back to the host entries"
    live.remove([0])
    live.replace([2], [3])


def test_every_scan_form_on_a_replacement(search_mode):
    pool = _pool(11, 11, kept=900)
    live = Live(pool)
    live.add(list(range(9)))
    live.replace([3], [9])
    form = capi.scan_last_launch()[0]
    live.replace([0, 8], [10, 3])
    want = {"generic": 1, "band": 2, "sampled-mfma": 4}.get(search_mode, 3)
    assert form == want, (search_mode, form)


def test_seeded_random_adds_removes_and_replaces_with_endings():
    pool = _pool(41, 24, kept=500, endings=True, min_s=15, padding=0.25, ts_shift=(0, 5, 17))
    rng = np.random.default_rng(43)
    live = Live(pool)
    live.add([int(x) for x in rng.choice(24, 14, replace=False)])
    ops = 0
    while ops < 42:
        n = len(live.cur)
        spare = [p for p in range(24) if p not in live.cur]
        kind = rng.integers(0, 3)
        if kind == 0 and n < 20 and spare:
            k = int(rng.integers(1, min(3, 20 - n, len(spare)) + 1))
            live.add([int(x) for x in rng.choice(spare, k, replace=False)])
        elif kind == 1 and n > 12:
            k = int(rng.integers(1, min(3, n - 12) + 1))
            live.remove([int(x) for x in rng.choice(n, k, replace=False)])
        elif kind == 2 and spare:
            k = int(rng.integers(1, min(3, len(spare)) + 1))
            live.replace([int(x) for x in rng.choice(n, k, replace=False)], [int(x) for x in rng.choice(spare, k, replace=False)])
        else:
            continue
        ops += 1


def test_failed_edits_leave_the_index_as_it_was():
    # a replacement without ending data while endings are on: the error add gives
    pool = _pool(13, 9, endings=True, min_s=15)
    live = Live(pool)
    live.add(list(range(7)))
    live.remove([2])
    before = live.state()
    no_ending = capi.FrameHashes.new(pool.o[7].opening, [], HD)
    with pytest.raises(capi.NeedleError) as e:
        live.index.replace([1], [no_ending])
    assert "no ending hash data" in str(e.value)
    assert live.state() == before
    with pytest.raises(capi.NeedleError) as e:
        live.index.remove([1, 1])
    assert e.value.name == "InvalidArgument" and live.state() == before
    with pytest.raises(capi.NeedleError) as e:
        live.index.replace([0, 0], [pool.c[7], pool.c[8]])
    assert e.value.name == "InvalidArgument" and live.state() == before
    live.replace([1], [7])           # the next valid operation still matches the oracle
    live.remove([0])


def _underflow_pool():
    """u shares an early segment E with y and a long late one with x; y shares E with u and a long late one with z.  With
    x present u's winner is the late segment; once x is removed it is E, whose end lies before the padding: the
    reference's subtraction overflows (y keeps its late winner with z, so the list with x searches fine)."""
    rng = np.random.default_rng(47)
    pool = Corpus(min_s=10, padding=20.0)
    rows = [rng.integers(0, 2 ** 32, 600, dtype=np.uint64).astype(np.uint32) for _ in range(5)]
    seg_e, seg_1, seg_2 = (rng.integers(0, 2 ** 32, L, dtype=np.uint64).astype(np.uint32) for L in (55, 200, 200))
    u, y, x, z, w = rows
    u[5:60] = y[5:60] = seg_e
    u[300:500] = x[300:500] = seg_1
    y[300:500] = z[300:500] = seg_2
    w[300:500] = seg_1 ^ seg_2      # a bystander that matches nothing
    for r in (u, y, x, z, w):
        pool.add_rows(r)
    return pool


def test_a_removal_whose_new_winner_underflows_fails_and_changes_nothing():
    pool = _underflow_pool()
    O.run_with_frame_hashes(pool.oracle_comparator(), pool.o)          # the whole list searches fine
    with pytest.raises(OverflowError):
        O.run_with_frame_hashes(pool.oracle_comparator(), [pool.o[p] for p in (0, 1, 3, 4)])
    live = Live(pool)
    live.add([0, 1, 2, 3, 4])
    before = live.state()
    with pytest.raises(capi.NeedleError):
        live.index.remove([2])
    assert live.state() == before
    live.remove([4])                 # the next valid operations still match the oracle
    live.remove([0, 2])              # u and x together: y keeps its late winner with z
