"""-m gpu: the library job pipeline with DIFFERENT data in flight (needle_hip_library_job_begin / _end, two slots).

Job k + 1's f32 first pass runs on a second stream beside job k's tail, and a lot is shared between the two jobs and
between libraries: the fingerprint pipes (chroma, energy, certification control, chunk and item lists, events) and
descriptor slots per device and job slot, the epilogue workspace with its host-side row-table caches per (device, slot),
the search workspace per device.  Every other test that puts two jobs in flight gives both the same PCM, which hides a
tail kernel reading the other pipe's chroma, a first pass starting before its pipe's previous reader finished, a row
table or descriptor table that is not replaced.  Here libraries that differ in geometry, step, channels, endings and
content (tests/pipeline_worker.py) share the pipeline, and every job -- hashes in the arena, complete run list with both
simhashes, per-video results -- is checked against the oracle."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests import pipeline_worker as W
from tests.test_gpu_certified import _near_threshold_pairs
from tests.test_gpu_scan_threshold import _min_len_for

pytestmark = pytest.mark.gpu
NS = O.NS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = max(1, min(16, len(os.sched_getaffinity(0))))
SNIPPET = 4096 + 19 * 1365                    # one raw item: 20 frames


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


class Ref:
    """The oracle's view of one library: hashes and timestamps per row, and -- per comparator -- the complete run list
    (with both simhashes) and the per-video results."""

    def __init__(self, spec):
        self.spec = spec
        ch, hd = spec.channels, O.duration_from_secs_f32(spec.hash_duration)
        self.hd = hd
        if spec.opening == 1.0:
            fhs = O.analyze_batch(spec.pcm, ch, hd, threads=THREADS)
        elif not spec.endings:
            fhs = O.analyze_batch([p[: ch * W.opening_samples(len(p) // ch)] for p in spec.pcm], ch, hd, threads=THREADS)
        else:                                                # the endings recipe of test_gpu_multi._oracle
            fhs = []
            for p in spec.pcm:
                dur = O.duration_from_secs_f64((len(p) // ch) * (1.0 / 11025.0))
                n_open = O.duration_mul_f32(dur, 0.5) * 11025 // NS
                seek = O.duration_mul_f32(dur, float(np.float32(1.0) - np.float32(0.25)))
                first = seek * 11025 // NS
                op = O.step_and_timestamp(O.fingerprint(p[: ch * n_open], ch), hd)
                en = O.step_and_timestamp(O.fingerprint(p[ch * first:], ch), hd, seek_to_ns=seek)
                fhs.append(O.FrameHashes(op, en, hd, ""))
        self.fhs = fhs
        regions = (lambda f: [f.opening, f.ending]) if spec.endings else (lambda f: [f.opening])
        self.rows = [[[h for h, _ in reg] for reg in regions(f)] for f in fhs]
        self.ts = [[[t for _, t in reg] for reg in regions(f)] for f in fhs]
        self._cache = {}

    def comparator(self, thr=10, min_s=None, padding=0.0):
        min_s = self.spec.min_s if min_s is None else min_s
        return O.Comparator(include_endings=self.spec.endings, hash_match_threshold=thr, min_opening_duration=min_s * NS,
                            min_ending_duration=min_s * NS, time_padding=O.duration_from_secs_f32(padding))

    def want(self, thr=10, min_s=None, padding=0.0):
        """(results as [[opening, ending]], sorted run list [k, 6]) for this comparator."""
        key = (thr, min_s, padding)
        if key not in self._cache:
            cmp = self.comparator(thr, min_s, padding)
            res = O.run_with_frame_hashes(cmp, self.fhs, threads=THREADS)
            self._cache[key] = ([None if r is None else [None if r.opening is None else list(r.opening),
                                                         None if r.ending is None else list(r.ending)] for r in res],
                                self._runs(thr, (cmp.min_opening_duration, cmp.min_ending_duration)))
        return self._cache[key]

    def _runs(self, thr, min_ns):
        """The oracle's table-free scan, pair by pair and region by region (problem = pair * regions + region), each
        pair at max(min run length of its two rows), the simhashes of both ends as in test_gpu_scan_threshold."""
        n, Rc = self.spec.n, len(self.rows[0])
        out, p = [], 0
        for i in range(n):
            for j in range(i + 1, n):
                for r in range(Rc):
                    a, b = (_min_len_for(self.ts[v][r], min_ns[r]) for v in (i, j))
                    if a == 0 or b == 0:
                        continue
                    src, dst = (np.array(self.rows[v][r], dtype=np.uint32) for v in (i, j))
                    total, runs = O.diagonal_runs_all_pairs([src, dst], thr, max(a, b), capacity=1 << 14)
                    if total > len(runs):
                        total, runs = O.diagonal_runs_all_pairs([src, dst], thr, max(a, b), capacity=total)
                    for _, i_end, j_end, ln in runs.tolist():
                        out.append((p * Rc + r, i_end, j_end, ln,
                                    O.simhash32(self.rows[i][r][i_end - ln:i_end + 1]),
                                    O.simhash32(self.rows[j][r][j_end - ln:j_end + 1])))
                p += 1
        keys = np.array(out, dtype=np.int64).reshape(-1, 6)
        return keys[np.lexsort(keys.T[::-1])]


def _res(rs):
    return [None if r is None else [None if r.opening is None else list(r.opening),
                                    None if r.ending is None else list(r.ending)] for r in rs]


def check_job(ref, lib, slot, res, found, thr=10, min_s=None, padding=0.0, what=""):
    """One finished job against the oracle: results, the complete run list, every row of the arena."""
    want_res, want_runs = ref.want(thr, min_s, padding)
    assert _res(res) == want_res, (ref.spec.name, slot, what)
    runs = W.sorted_runs(lib.job_runs(slot))
    assert found == len(runs) == len(want_runs), (ref.spec.name, slot, what, found, len(runs), len(want_runs))
    assert np.array_equal(runs, want_runs), (ref.spec.name, slot, what)
    assert W.arena_rows(lib, ref.spec) == ref.rows, (ref.spec.name, slot, what)


# ---- the libraries ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    out = {"a": Ref(W.spec_a()), "b": Ref(W.spec_b()), "c": Ref(W.spec_c())}
    kept_a = len(out["a"].rows[0][0])
    assert all(len(r[0]) == kept_a for r in out["a"].rows)
    assert kept_a == int(capi.lib().needle_hip_fingerprint_num_kept(W.opening_samples(len(out["a"].spec.pcm[0])), 2))
    out["d"] = Ref(W.spec_d(kept_a))
    out["h"] = Ref(W.spec_h())
    out["h"].spec.device.free()
    a, b, c, d = (out[k] for k in "abcd")
    # what makes each one a probe: B another count, step, channel count and endings; C A's geometry, other hashes; D A's
    # row lengths (row-table sizes), other timestamps; H silence and chords: large buckets, many recomputations
    assert b.spec.n != a.spec.n and len({len(p) for p in b.spec.pcm}) == b.spec.n and b.spec.channels == 2
    assert [len(p) for p in c.spec.pcm] == [len(p) for p in a.spec.pcm] and c.rows != a.rows
    assert [[len(x) for x in r] for r in d.rows] == [[len(x) for x in r] for r in a.rows]
    assert d.ts[0][0] != a.ts[0][0] and d.rows != a.rows
    for ref in out.values():                                   # every job below must find something
        res, runs = ref.want()
        assert len(runs) > 0 and sum(1 for r in res if r is not None and r[0] is not None) >= 2, ref.spec.name
    assert any(r is not None and r[1] is not None for r in b.want()[0])
    return out


@pytest.fixture(scope="module")
def near():
    """Near-threshold PCM snippets (one raw item each) that the certified first pass must send to the f64 path."""
    pairs = _near_threshold_pairs(12, seed=29)
    assert len(pairs) >= 10
    return [p for lo, hi, *_ in pairs for p in (lo, hi)]


@pytest.fixture(scope="module")
def ref_x(near):
    """Library X: 8 episodes of 60 s, openings at step 2, with the near-threshold snippets planted at sample offsets
    k * 1365, k even: each snippet is exactly kept item k / 2 of its episode."""
    eps = synth.make_library(8, 60.0, 15.0, seed_base=synth.EPISODE_SEED ^ 0x7)
    pcm, planted = [], []
    for v, e in enumerate(eps):
        p = e.pcm.copy()
        for s in range(3):
            idx = 3 * v + s
            if idx >= len(near):
                break
            k = 2 * (4 + 12 * s + v)                           # in the opening half, 24 frames apart: clear of each other
            p[k * 1365:k * 1365 + SNIPPET] = near[idx]
            planted.append((v, k // 2, int(O.fingerprint(near[idx])[0])))
        pcm.append(p)
    ref = Ref(W.Spec("x", pcm, 1, 0.3))
    for v, kept, item in planted:
        assert ref.rows[v][0][kept] == item
    ref.planted = planted
    return ref


def _libs(refs, names):
    return {k: refs[k].spec.library() if refs[k].spec.device is None else _device_library(refs[k]) for k in names}


def _device_library(ref):
    gen = synth.DeviceLibrary(ref.spec.n, len(ref.spec.pcm[0]), 40.0, hostile=True)
    lib = capi.Library(ref.spec.n, opening_search_percentage=1.0)
    lib.set_pcm_device(gen.pointers(), [len(p) for p in ref.spec.pcm])
    gen.free()
    return lib


# ---- 1. two libraries in flight, every slot pairing --------------------------------------------------------------------
@pytest.mark.parametrize("device_epilogue", ["0", "1"])
def test_two_libraries_in_flight_every_slot_pairing(refs, monkeypatch, device_epilogue):
    monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", device_epilogue)
    libs = _libs(refs, "abcd")
    cmps = {k: refs[k].spec.comparator() for k in "abcd"}
    seen = []

    def on_end(name, slot, lib, res, found):
        assert lib.job_form(slot)["device_epilogue"] == (device_epilogue == "1")
        check_job(refs[name], lib, slot, res, found, what=f"job {len(seen)}")
        seen.append((name, slot))

    W.run_schedule(libs, cmps, {"P": "a", "Q": "b", "R": "c", "S": "d"}, on_end)
    assert len(seen) == W.ROUNDS * sum(1 for op, _, _ in W.ROUND if op == "e")
    assert {(n, s) for n, s in seen} >= {("a", 0), ("a", 1), ("b", 0), ("b", 1), ("c", 0), ("c", 1), ("d", 0)}


# ---- 2. one library, two comparators in flight -------------------------------------------------------------------------
@pytest.mark.parametrize("thr1,mfma", [(16, False), (3, True)])
def test_one_library_two_comparators_in_flight(refs, monkeypatch, thr1, mfma):
    a = refs["a"]
    lib = a.spec.library()
    c0 = capi.Comparator([f"a{k}.wav" for k in range(a.spec.n)], hash_match_threshold=10, min_opening_duration=10)
    c1 = capi.Comparator([f"a{k}.wav" for k in range(a.spec.n)], hash_match_threshold=thr1, min_opening_duration=20,
                         time_padding=1.5)
    k0, k1 = dict(thr=10, min_s=10), dict(thr=thr1, min_s=20, padding=1.5)

    def begin(cmp, slot):
        if slot == 1 and mfma:
            monkeypatch.setenv("NEEDLE_HIP_SCAN_MFMA", "1")
        lib.job_begin(cmp, slot)
        monkeypatch.delenv("NEEDLE_HIP_SCAN_MFMA", raising=False)

    forms = {}
    for cmp, slot in ((c0, 0), (c1, 1)):                       # each alone: the form it takes by itself
        begin(cmp, slot)
        lib.job_end(cmp, slot)
        forms[slot] = lib.job_form(slot)["scan_form"]
    if mfma:
        assert forms[1] == 4
    assert forms[0] != forms[1] or not mfma
    begin(c0, 0)
    begin(c1, 1)
    res0, f0 = lib.job_end(c0, 0)
    check_job(a, lib, 0, res0, f0, **k0)
    runs0 = lib.job_runs(0)
    res1, f1 = lib.job_end(c1, 1)
    check_job(a, lib, 1, res1, f1, **k1)
    assert lib.job_form(0)["scan_form"] == forms[0] and lib.job_form(1)["scan_form"] == forms[1]
    begin(c1, 1)                                              # needle_hip.h: slot 0's list stays valid until ITS next begin
    assert np.array_equal(lib.job_runs(0), runs0)
    begin(c0, 0)
    res1, f1 = lib.job_end(c1, 1)
    check_job(a, lib, 1, res1, f1, **k1)
    res0, f0 = lib.job_end(c0, 0)
    check_job(a, lib, 0, res0, f0, **k0)
    assert lib.job_form(0)["scan_form"] == forms[0] and lib.job_form(1)["scan_form"] == forms[1]
    assert a.want(**k0)[0] != a.want(**k1)[0] or len(a.want(**k0)[1]) != len(a.want(**k1)[1])


# ---- 3. recomputed items beside a neighbour ----------------------------------------------------------------------------
def test_recomputed_items_beside_a_hostile_neighbour(refs, ref_x, near):
    x, h = ref_x, refs["h"]
    capi.cert_stats(reset=True)
    got = capi.fingerprint(near, step=1)                      # each snippet alone: refused by the first pass, recomputed
    st = capi.cert_stats(reset=True)
    assert [g.tolist() for g in got] == [O.fingerprint(p).tolist() for p in near]
    assert st["items"] == st["items_recomputed"] == len(near), st
    libs = {"x": x.spec.library(), "h": _device_library(h)}
    cmps = {k: r.spec.comparator() for k, r in (("x", x), ("h", h))}
    solo = {}
    for name, slot in (("x", 0), ("h", 1)):                  # alone: how many items each job recomputes
        capi.cert_stats(reset=True)
        libs[name].job_begin(cmps[name], slot)
        res, found = libs[name].job_end(cmps[name], slot)
        check_job(x if name == "x" else h, libs[name], slot, res, found, what="alone")
        solo[name] = capi.cert_stats(reset=True)["items_recomputed"]
    assert solo["x"] >= len(x.planted) and solo["h"] > solo["x"], solo
    for order in ([("h", 0), ("x", 1)], [("h", 1), ("x", 0)], [("x", 0), ("h", 1)], [("x", 1), ("h", 0)]):
        for _ in range(2):
            capi.cert_stats(reset=True)
            for name, slot in order:
                libs[name].job_begin(cmps[name], slot)
            for name, slot in order[::-1] if order[0][0] == "h" else order:
                res, found = libs[name].job_end(cmps[name], slot)
                check_job(x if name == "x" else h, libs[name], slot, res, found, what=str(order))
            st = capi.cert_stats(reset=True)
            assert st["items_recomputed"] == solo["x"] + solo["h"], (order, st, solo)
            hx = W.arena_rows(libs["x"], x.spec)
            for v, kept, item in x.planted:
                assert hx[v][0][kept] == item, (order, v, kept)


# ---- 4. other device calls between job_begin and job_end ---------------------------------------------------------------
def test_other_device_calls_while_a_job_is_in_flight(refs):
    a = refs["a"]
    lib = a.spec.library()
    cmp = a.spec.comparator()
    other = [e.pcm for e in synth.make_library(3, 47.0 + 0.0, 9.0, seed_base=0xAB12)]
    other[1] = other[1][: len(other[1]) - 777]
    rows = [O.fingerprint(p)[::2] for p in other]
    fhs_o = [O.FrameHashes(O.step_and_timestamp(O.fingerprint(p), a.hd), [], a.hd, "") for p in other]
    stereo44 = np.repeat(other[0][:200_000], 2)
    idx_cmp = capi.Comparator([f"o{k}.wav" for k in range(3)], min_opening_duration=3)
    for slot in (0, 1, 0):
        lib.job_begin(cmp, slot)
        for step in (1, 2, 4, 8):
            got = capi.fingerprint(other, step=step)
            assert [g.tolist() for g in got] == [O.fingerprint(p)[::step].tolist() for p in other], step
        problems = [(0, 1, 20), (1, 2, 20), (0, 2, 35)]
        runs = capi.hamming_runs(rows, problems, 10)
        got = sorted(zip(*(runs[f].tolist() for f in ("problem", "src_end", "dst_end", "len"))))
        want = []
        for q, (s, d, m) in enumerate(problems):
            total, r = O.diagonal_runs_all_pairs([rows[s], rows[d]], 10, m, capacity=1 << 14)
            want += [(q, i, j, ln) for _, i, j, ln in r.tolist()]
        assert got == sorted(want)
        assert capi.resample([stereo44], 2, 44100)[0].tolist() == O.resample(stereo44, 2, 44100).tolist()
        index = capi.Index(idx_cmp)
        index.add([capi.FrameHashes.new(f.opening, [], a.hd) for f in fhs_o])
        want_idx = O.run_with_frame_hashes(O.Comparator(min_opening_duration=3 * NS), fhs_o)
        assert _res(index.results()) == _res(want_idx)
        res, found = lib.job_end(cmp, slot)
        check_job(a, lib, slot, res, found, what=f"slot {slot} with other calls")


# ---- 5. first pass at larger steps -------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [3, 4, 5, 8, 63, 126, 127, 128, 200])
def test_first_pass_at_larger_steps(near, step):
    """items_per_tile = min(64, 126 / step + 1): 43, 32, 26, 16, 3, 2, 1, 1, 1 (127 and up: one item, a tile of more than
    the 142 LDS rows' worth of frames); mono and stereo, ragged batches, near-threshold items."""
    eps = [synth.make_episode(k, 40.0 + 23.3 * k, 10.0, seed_base=0x5 + step) for k in range(4)]
    mono = [e.pcm for e in eps] + [eps[0].pcm[:SNIPPET + 1365 * step], eps[1].pcm[:4096 + 1365 * 19 - 1]] + near[:6]
    got = capi.fingerprint(mono, step=step)
    assert [g.tolist() for g in got] == [O.fingerprint(p)[::step].tolist() for p in mono]
    assert max(len(g) for g in got) >= 4 and len(got[-1]) == 1 and len(got[5]) == 0
    rng = np.random.default_rng(step)
    stereo = []
    for p in mono[:4] + near[6:10]:
        s = np.repeat(p, 2)
        s[1::2] = np.clip(s[1::2].astype(np.int32) + rng.integers(-5, 6, len(p)), -32768, 32767)
        stereo.append(s)
    got = capi.fingerprint(stereo, channels=2, step=step)
    assert [g.tolist() for g in got] == [O.fingerprint(s, 2)[::step].tolist() for s in stereo]
    # the planted items at kept positions of a longer stream: item k * step of a stream is its kept item k
    long = eps[3].pcm.copy()
    at = []
    for q, p in enumerate(near[10:14]):
        k = step * -(-24 // step) * (q + 1)                    # >= 24 frames apart: the snippets do not overlap
        if k * 1365 + SNIPPET > len(long):
            break
        long[k * 1365:k * 1365 + SNIPPET] = p
        at.append((k // step, int(O.fingerprint(p)[0])))
    g = capi.fingerprint([long], step=step)[0]
    assert g.tolist() == O.fingerprint(long)[::step].tolist()
    assert all(int(g[k]) == item for k, item in at) and at


# ---- 6. pipeline modes, in fresh processes ---------------------------------------------------------------------------
MODES = {"default": {}, "share1": {"NEEDLE_HIP_STFT_SHARE": "1"}, "share0": {"NEEDLE_HIP_STFT_SHARE": "0"},
         "priority0": {"NEEDLE_HIP_LIBRARY_PRIORITY": "0"}}
_child_failed = []


@pytest.mark.parametrize("mode", list(MODES))
def test_pipeline_modes_in_a_fresh_process(refs, tmp_path, mode):
    assert not _child_failed, f"an earlier child ended abnormally ({_child_failed}): no further child is started"
    env = {k: v for k, v in os.environ.items() if k not in ("NEEDLE_HIP_STFT_SHARE", "NEEDLE_HIP_LIBRARY_PRIORITY",
                                                            "NEEDLE_HIP_DEVICE_EPILOGUE", "NEEDLE_HIP_TRACE")}
    env.update(MODES[mode], NEEDLE_HIP_TRACE="1")
    out = tmp_path / "jobs.json"
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pipeline_worker.py"), str(out)], env=env,
                           capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        _child_failed.append((mode, "timeout"))
        raise
    if p.returncode != 0:
        _child_failed.append((mode, p.returncode))
    assert p.returncode == 0, (mode, p.returncode, p.stderr[-3000:])
    jobs = json.load(open(out))["jobs"]
    assert len(jobs) == W.ROUNDS * sum(1 for op, _, _ in W.ROUND if op == "e")
    for k, job in enumerate(jobs):
        ref = refs[job["lib"]]
        want_res, want_runs = ref.want()
        assert job["results"] == want_res, (mode, k, job["lib"], job["slot"])
        assert job["found"] == len(want_runs) and np.array_equal(np.array(job["runs"], dtype=np.int64).reshape(-1, 6),
                                                                 want_runs), (mode, k, job["lib"])
        assert job["rows"] == ref.rows, (mode, k, job["lib"])
    # which first passes ran beside the other pipe (NEEDLE_HIP_TRACE), counting each library's jobs after its first
    current, begun, beside, passes = None, set(), 0, 0
    for line in p.stderr.splitlines():
        m = re.match(r"\[pipeline_worker\] job_begin (\w+) (\d)", line)
        if m:
            current = (m.group(1), m.group(1) in begun)
            begun.add(m.group(1))
        elif line.startswith("[needle_hip] pipelined first pass:") and current is not None:
            passes += 1
            beside += current[1] and "beside the other pipe" in line
    if mode == "share0":
        assert passes == 0                                     # one stream: no pipelined first pass at all
    else:
        assert passes >= len(jobs)
    if mode == "default":
        assert beside >= 1, "no job of the schedule ran its first pass beside the other pipe"
    print(f"pipeline mode {mode}: {passes} pipelined first passes, {beside} beside the other pipe (after each library's first)")
