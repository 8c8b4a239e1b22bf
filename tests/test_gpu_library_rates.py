"""Library PCM at decode rates on the MI355X: needle_hip_library_set_sample_rate through set_pcm, set_pcm_device and
stream_pcm, every resampler kernel family, windows resampled in pieces, two simulated ranks, the unchanged default and
configs[1]'s scale, against the oracle (a window cut at the source rate -> oracle.resample -> oracle.fingerprint ->
step_and_timestamp, with the ending's seek) and against Analyzer.run_pcm at the same rate."""
import os

import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests.test_multichannel_cpu import surround

pytestmark = pytest.mark.gpu
NS = O.NS
HD = 0.3
ENDING = 0.25


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def at_rate(mono, rate, ch, k):
    """An 11025 Hz episode brought to `rate` (sample-and-hold, so the content survives the resampler) in `ch` channels
    that differ: stereo adds a quieter, noisier right channel; 3-8 channels are oracle-test surround."""
    idx = (np.arange(int(len(mono) * rate / 11025), dtype=np.int64) * 11025) // rate
    up = mono[idx]
    if ch == 1:
        return up
    if ch == 2:
        rng = np.random.default_rng(k)
        right = np.clip(up.astype(np.int32) // 2 + rng.integers(-300, 300, len(up)), -32768, 32767).astype(np.int16)
        return np.stack([up, right], axis=1).reshape(-1)
    return surround(up, ch, k)


def windows(n_values, ch, rate, endings=True):
    """(first frame, frames) of the opening window and, with endings, (first frame, frames, seek ns) of the ending
    window: Analyzer::windows at the source rate."""
    frames = n_values // ch
    dur = O.duration_from_secs_f64(frames * (1.0 / rate))
    n_open = min(O.duration_mul_f32(dur, 0.5) * rate // NS, frames)
    seek = O.duration_mul_f32(dur, float(np.float32(1.0) - np.float32(ENDING)))
    first = min(seek * rate // NS, frames)
    return (0, n_open), (first, frames - first, seek)


def oracle_frame_hashes(pcm, ch, rate, endings=True):
    hd = O.duration_from_secs_f32(HD)
    (o0, on), (e0, en, seek) = windows(len(pcm), ch, rate)
    op = O.step_and_timestamp(O.fingerprint(O.resample(pcm[ch * o0: ch * (o0 + on)], ch, rate)), hd)
    ed = O.step_and_timestamp(O.fingerprint(O.resample(pcm[ch * e0: ch * (e0 + en)], ch, rate)), hd,
                              seek_to_ns=seek) if endings else []
    return O.FrameHashes(op, ed, hd)


def hashes_of(fh):
    h, ts = fh.opening_data()
    eh, ets = fh.ending_data()
    return h.tolist(), ts.tolist(), eh.tolist(), ets.tolist()


def oracle_hashes(f):
    return [h for h, _ in f.opening], [t for _, t in f.opening], [h for h, _ in f.ending], [t for _, t in f.ending]


def results(rs):
    return [None if r is None else (r.opening, r.ending) for r in rs]


def job(lib, cmp):
    lib.job_begin(cmp, 0)
    res, _ = lib.job_end(cmp, 0)
    return res, lib.job_runs(0)


def sorted_runs(runs):
    return np.sort(runs, order=["problem", "src_end", "dst_end"])


def device_copies(pcms):
    """The streams in device buffers, each starting 2 bytes past a 16-byte boundary."""
    L = capi.lib()
    bufs, ptrs = [], []
    for p in pcms:
        b = capi.DeviceBuffer(p.nbytes + 16)
        capi.check(L.needle_hip_memcpy_h2d(b.ptr + 2, p.ctypes.data, p.nbytes))
        bufs.append(b)
        ptrs.append(b.ptr + 2)
    return bufs, ptrs


def new_library(n, rate):
    return capi.Library(n).include_endings(ENDING).set_sample_rate(rate)


@pytest.fixture(scope="module")
def episodes():
    return synth.make_library(5, 90.0, 20.0, outro_s=15.0)


# rate, channels: the kernel family each takes (resample.hip): integer decimation 44.1 / 22.05 kHz, matrix cores
# 48 / 32 kHz, DPP quads 96 kHz, the general kernel 12345 Hz
FAMILIES = [(44100, 2), (22050, 1), (48000, 2), (48000, 6), (32000, 1), (96000, 2), (12345, 1)]


@pytest.mark.parametrize("rate,ch", FAMILIES)
def test_every_kernel_family_through_every_entry_point(episodes, rate, ch):
    n = len(episodes)
    pcms = [at_rate(e.pcm, rate, ch, k) for k, e in enumerate(episodes)]
    lens = [len(p) for p in pcms]
    ref = [oracle_frame_hashes(p, ch, rate) for p in pcms]
    want = O.run_with_frame_hashes(O.Comparator(include_endings=True, min_opening_duration=10 * NS,
                                                min_ending_duration=10 * NS), ref)
    assert sum(w is not None and w.opening is not None for w in want) >= 3
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(n)], include_endings=True, min_opening_duration=10,
                          min_ending_duration=10)
    analyzer = (capi.Analyzer.from_files([f"ep{k}.wav" for k in range(n)]).with_include_endings(True)
                .with_ending_search_percentage(ENDING).run_pcm(pcms, channels=ch, sample_rate=rate))

    lib = new_library(n, rate)
    lib.set_pcm(pcms, lens, channels=ch)
    got, runs = job(lib, cmp)
    assert results(got) == results(want)
    for v in range(n):
        assert hashes_of(lib.frame_hashes(v)) == oracle_hashes(ref[v]) == hashes_of(analyzer[v]), v
    audit = lib.audit()
    assert audit["mismatches"] == 0 and audit["accepted_mismatches"] == 0
    del lib

    bufs, ptrs = device_copies(pcms)
    dev = new_library(n, rate)
    dev.set_pcm_device(ptrs, lens, channels=ch)
    del bufs                                                                   # the caller's buffers are free on return
    got_d, runs_d = job(dev, cmp)
    assert results(got_d) == results(want)
    assert np.array_equal(sorted_runs(runs_d), sorted_runs(runs))
    for v in range(n):
        assert hashes_of(dev.frame_hashes(v)) == oracle_hashes(ref[v]), v
    audit = dev.audit()
    assert audit["mismatches"] == 0 and audit["accepted_mismatches"] == 0
    del dev

    st = new_library(n, rate)
    st.stream_pcm(pcms, lens, channels=ch)
    got_s, runs_s = job(st, cmp)
    assert results(got_s) == results(want)
    assert np.array_equal(sorted_runs(runs_s), sorted_runs(runs))
    for v in range(n):
        assert hashes_of(st.frame_hashes(v)) == oracle_hashes(ref[v]), v


PIECES = [(44100, 2, {}), (22050, 1, {}), (48000, 2, {}), (48000, 6, {}), (96000, 2, {}), (12345, 1, {}),
          (48000, 2, {"NEEDLE_HIP_RESAMPLE_QUAD": "1"}), (48000, 2, {"NEEDLE_HIP_RESAMPLE_V1": "1"})]


@pytest.mark.parametrize("rate,ch,env", PIECES)
def test_windows_resampled_in_pieces(episodes, monkeypatch, rate, ch, env):
    """set_pcm with a staging buffer of a few thousand values: every window is resampled in many pieces of whole
    tiles (and set_pcm_device of 6 channels down-mixes in pieces too); the hashes equal the unpieced library's and the
    oracle's."""
    eps = episodes[:3]
    n = len(eps)
    pcms = [at_rate(e.pcm, rate, ch, k) for k, e in enumerate(eps)]
    lens = [len(p) for p in pcms]
    ref = [oracle_hashes(oracle_frame_hashes(p, ch, rate)) for p in pcms]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    whole = new_library(n, rate)
    whole.set_pcm(pcms, lens, channels=ch)
    whole.analyze(0, n)
    monkeypatch.setenv("NEEDLE_HIP_MAX_BATCH_VALUES", "3001")
    pieces = new_library(n, rate)
    pieces.set_pcm(pcms, lens, channels=ch)
    pieces.analyze(0, n)
    bufs, ptrs = device_copies(pcms)
    dev = new_library(n, rate)
    dev.set_pcm_device(ptrs, lens, channels=ch)
    del bufs
    dev.analyze(0, n)
    for v in range(n):
        assert hashes_of(pieces.frame_hashes(v)) == hashes_of(whole.frame_hashes(v)) == ref[v], v
        assert hashes_of(dev.frame_hashes(v)) == ref[v], v


def test_two_simulated_ranks_at_48k_stereo():
    """rank_videos at 48 kHz picks each rank's videos; two Library objects standing in for two ranks hold only those
    videos' PCM and fingerprint them; their rows together give the oracle's results."""
    n, world, ch, rate = 7, 2, 2, 48000
    eps = synth.make_library(n, 90.0, 20.0)
    pcms = [at_rate(e.pcm, rate, ch, k) for k, e in enumerate(eps)]
    lens = [len(p) for p in pcms]
    ref = [oracle_frame_hashes(p, ch, rate, endings=False) for p in pcms]
    for f in ref:
        f.ending = []
    want = O.run_with_frame_hashes(O.Comparator(min_opening_duration=10 * NS), ref)
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(n)], min_opening_duration=10)
    L = capi.lib()
    plans = [capi.Library(n).set_sample_rate(rate).rank_videos(lens, world, r, channels=ch) for r in range(world)]
    assert plans[0][0] == 0 and plans[-1][0] + plans[-1][1] == n and all(c > 0 for _, c in plans)
    libs = []
    for first, count in plans:
        lib = capi.Library(n).set_sample_rate(rate)
        lib.set_pcm([p if first <= k < first + count else None for k, p in enumerate(pcms)], lens, channels=ch)
        lib.analyze(first, count)
        arena, stride = lib.hash_arena()
        libs.append((lib, arena, stride))
    stride = libs[0][2]
    full = np.zeros((n, stride), dtype=np.uint32)
    for (lib, arena, _), (first, count) in zip(libs, plans):
        rows = np.zeros(n * stride, dtype=np.uint32)
        capi.check(L.needle_hip_memcpy_d2h(rows.ctypes.data, arena, rows.nbytes))
        full[first:first + count] = rows.reshape(n, stride)[first:first + count]
    for v in range(n):
        assert full[v][: len(ref[v].opening)].tolist() == [h for h, _ in ref[v].opening], v
    lib0, arena0, _ = libs[0]
    capi.check(L.needle_hip_memcpy_h2d(arena0, full.ctypes.data, full.nbytes))
    cap = 4096
    d_runs, d_count = capi.DeviceBuffer(cap * capi.RUN_DTYPE.itemsize), capi.DeviceBuffer(4)
    lib0.search(cmp, 0, lib0.num_pairs(), d_runs.ptr, cap, d_count.ptr, sync=True)
    runs = d_runs.to_host(capi.RUN_DTYPE, int(d_count.to_host(np.uint32, 1)[0]))
    assert results(lib0.finalize(cmp, runs)) == results(want)


def test_default_rate_is_unchanged_and_the_setter_comes_first():
    n = 5
    eps = synth.make_library(n, 90.0, 20.0)
    pcms = [np.repeat(e.pcm, 2) for e in eps]
    lens = [len(p) for p in pcms]
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(n)], min_opening_duration=10)
    plain = capi.Library(n)
    plain.set_pcm(pcms, lens, channels=2)
    got_p, runs_p = job(plain, cmp)
    explicit = capi.Library(n).set_sample_rate(11025)
    explicit.set_pcm(pcms, lens, channels=2)
    got_e, runs_e = job(explicit, cmp)
    assert results(got_e) == results(got_p)
    assert np.array_equal(sorted_runs(runs_e), sorted_runs(runs_p))
    for v in range(n):
        assert hashes_of(explicit.frame_hashes(v)) == hashes_of(plain.frame_hashes(v))
    with pytest.raises(capi.NeedleError):
        explicit.set_sample_rate(48000)                                        # after set_pcm: refused ...
    got_again, runs_again = job(explicit, cmp)                                 # ... and the library unchanged
    assert results(got_again) == results(got_p)
    assert np.array_equal(sorted_runs(runs_again), sorted_runs(runs_p))


def test_config1_scale_at_48k_stereo():
    """28 x 24 min at 48 kHz stereo (7.7 GB of PCM) through stream_pcm and set_pcm: every video's opening hashes equal
    Analyzer.run_pcm at 48 kHz, three videos' equal the oracle's, and the two entry points find the same runs."""
    n, ch, rate = 28, 2, 48000
    eps = synth.make_library(n, 24 * 60.0, 90.0)
    pcms = [at_rate(e.pcm, rate, ch, k) for k, e in enumerate(eps)]
    del eps
    lens = [len(p) for p in pcms]
    fhs = capi.Analyzer.from_files([f"ep{k}.wav" for k in range(n)]).run_pcm(pcms, channels=ch, sample_rate=rate)
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(n)])
    st = capi.Library(n).set_sample_rate(rate)
    st.stream_pcm(pcms, lens, channels=ch)
    got_s, runs_s = job(st, cmp)
    res = capi.Library(n).set_sample_rate(rate)
    res.set_pcm(pcms, lens, channels=ch)
    got, runs = job(res, cmp)
    assert results(got) == results(got_s)
    assert np.array_equal(sorted_runs(runs), sorted_runs(runs_s))
    assert sum(r is not None and r.opening is not None for r in got) == n
    for v in range(n):
        want = fhs[v].opening_data()[0].tolist()
        assert res.frame_hashes(v).opening_data()[0].tolist() == want, v
        assert st.frame_hashes(v).opening_data()[0].tolist() == want, v
    hd = O.duration_from_secs_f32(HD)
    for v in (0, 13, n - 1):
        (o0, on), _ = windows(lens[v], ch, rate)
        o = O.step_and_timestamp(O.fingerprint(O.resample(pcms[v][: ch * on], ch, rate)), hd)
        assert res.frame_hashes(v).opening_data()[0].tolist() == [h for h, _ in o], v
