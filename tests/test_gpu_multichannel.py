"""3-8 channel (surround) PCM on the MI355X: the down-mix kernel against a truncating average, and every analyze path
that takes C-channel input -- fingerprint, resampler, Analyzer, the command line, the resident and streamed library --
against the oracle, which states the down-mix as (sum of a frame) / C with C truncation (oracle/ora_resample.h)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests.test_multichannel_cpu import surround, write_wav_multichannel

pytestmark = pytest.mark.gpu
NS = O.NS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _truncating_mean(x, ch):
    frames = len(x) // ch
    s = x[: frames * ch].reshape(frames, ch).astype(np.int32).sum(axis=1, dtype=np.int32)
    return (np.sign(s) * (np.abs(s) // ch)).astype(np.int16)


def test_downmix_equals_truncating_average(monkeypatch):
    """C = 3..8; streams of 0, 1, 7, 8, 9 and 2.5 M frames, with and without a partial trailing frame; all -32768,
    all 32767 and mixed-sign noise (negative sums C does not divide round toward zero); one batch of everything and
    the same cut into many small batches (NEEDLE_HIP_MAX_BATCH_VALUES)."""
    rng = np.random.default_rng(17)
    for ch in range(3, 9):
        pcms = []
        for frames in (0, 1, 7, 8, 9, 2_500_000 + ch):
            for extra in (0, ch - 1):
                pcms.append(rng.integers(-32768, 32768, frames * ch + extra, dtype=np.int64).astype(np.int16))
        pcms.append(np.full(1000 * ch + 1, -32768, np.int16))
        pcms.append(np.full(1001 * ch, 32767, np.int16))
        small = np.array([-7, 1, 0, 0, 0, 0, 0, 0], np.int16)[:ch]    # sum -6 ... -7 with small positive terms
        pcms.append(np.tile(np.concatenate([small, -small]), 37))
        want = [_truncating_mean(p, ch) for p in pcms]
        got = capi.downmix(pcms, ch)
        for g, w, p in zip(got, want, pcms):
            assert len(g) == len(p) // ch and np.array_equal(g, w), (ch, len(p))
        if ch in (3, 6, 8):
            monkeypatch.setenv("NEEDLE_HIP_MAX_BATCH_VALUES", str(4096 * ch + 5))
            for g, w in zip(capi.downmix(pcms, ch), want):
                assert np.array_equal(g, w), ch
            monkeypatch.delenv("NEEDLE_HIP_MAX_BATCH_VALUES")
    # the contract's exact values: -7 / 6 = -1, 6 x -32768 / 6 = -32768
    assert capi.downmix([np.array([-7, 0, 0, 0, 0, 0], np.int16)], 6)[0].tolist() == [-1]
    assert capi.downmix([np.full(6, -32768, np.int16)], 6)[0].tolist() == [-32768]
    with pytest.raises(capi.NeedleError):
        capi.downmix([np.zeros(18, np.int16)], 9)


def test_downmix_of_more_than_a_gibibyte_in_one_batch():
    ch = 6
    frames = 90_000_000                                               # 540 M values = 1.08 GB of s16
    x = np.random.default_rng(5).integers(-32768, 32768, frames * ch, dtype=np.int16)
    got = capi.downmix([x], ch)[0]
    assert np.array_equal(got, _truncating_mean(x, ch))


def _episode6(e, seed=0):
    return surround(e.pcm, 6, 1000 + seed)


def test_fingerprint_and_resampler_take_six_channels():
    eps = synth.make_library(2, 40.0, 12.0)
    pcm6 = [_episode6(e, k) for k, e in enumerate(eps)]
    assert not np.array_equal(capi.downmix([pcm6[0]], 6)[0], eps[0].pcm)         # the channels really differ
    got = capi.fingerprint(pcm6 + [pcm6[1][:6 * 50_000 + 5]], channels=6)
    for g, p in zip(got, pcm6 + [pcm6[1][:6 * 50_000 + 5]]):
        assert g.tolist() == O.fingerprint(p, channels=6).tolist()
    for rate in (44100, 48000):
        t = np.arange(rate * 7) / rate
        base = (8000 * np.sin(2 * np.pi * 330 * t)).astype(np.int16)
        pcms = [surround(base, 6, rate), surround(base[:777], 6, 3)[:-2], np.zeros(0, np.int16)]
        for g, p in zip(capi.resample(pcms, 6, rate), pcms):
            assert g.tolist() == O.resample(p, 6, rate).tolist(), rate
        fp = capi.fingerprint([O.resample(pcms[0], 6, rate)])[0]
        assert fp.tolist() == O.fingerprint(O.resample(pcms[0], 6, rate)).tolist()


def test_analyzer_run_pcm_six_channels_48k_with_endings():
    """Opening and ending windows of 6-channel 48 kHz streams: resampled on the device after the down-mix, hashes and
    timestamps (seek offsets included) equal oracle.resample -> oracle.fingerprint."""
    rate, ch = 48000, 6
    hd = O.duration_from_secs_f32(0.3)
    pcms = []
    for k in range(3):
        e = synth.make_episode(k, 30.0, 10.0)
        up = np.repeat(e.pcm, 4)[: int(len(e.pcm) * rate / 11025)]
        pcms.append(surround(up, ch, k))
    fhs = (capi.Analyzer.from_files([f"e{k}.wav" for k in range(3)]).with_include_endings(True)
           .with_ending_search_percentage(0.25).run_pcm(pcms, channels=ch, sample_rate=rate))
    for fh, p in zip(fhs, pcms):
        frames = len(p) // ch
        dur = O.duration_from_secs_f64(frames * (1.0 / rate))
        n_open = O.duration_mul_f32(dur, 0.5) * rate // NS
        seek = O.duration_mul_f32(dur, float(np.float32(1.0) - np.float32(0.25)))
        first = seek * rate // NS
        o = O.step_and_timestamp(O.fingerprint(O.resample(p[: ch * n_open], ch, rate)), hd)
        en = O.step_and_timestamp(O.fingerprint(O.resample(p[ch * first:], ch, rate)), hd, seek_to_ns=seek)
        h, ts = fh.opening_data()
        assert h.tolist() == [x for x, _ in o] and ts.tolist() == [t for _, t in o]
        h, ts = fh.ending_data()
        assert h.tolist() == [x for x, _ in en] and ts.tolist() == [t for _, t in en]


def test_cli_analyze_then_search_on_mixed_channel_counts(tmp_path):
    """`needle analyze <dir>` then `needle search <dir>` on 6-channel WAVs (16-bit, 24-bit extensible, float) mixed with
    mono and stereo ones: .needle.dat contents and the printed results equal the oracle's."""
    exe = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "bin", "needle")
    eps = synth.make_library(5, 90.0, 20.0)
    hd = O.duration_from_secs_f32(0.3)
    paths, ref = [], []
    layouts = [(6, "s16", False), (1, "s16", False), (6, "s24", True), (2, "s16", False), (6, "f32", False)]
    for k, (e, (ch, kind, ext)) in enumerate(zip(eps, layouts)):
        p = str(tmp_path / f"s01e0{k}.wav")
        pcm = e.pcm if ch == 1 else np.repeat(e.pcm, 2) if ch == 2 else _episode6(e, k)
        write_wav_multichannel(p, pcm, ch, kind=kind, extensible=ext)
        paths.append(p)
        frames = len(pcm) // ch
        dur = O.duration_from_secs_f64(frames * (1.0 / 11025.0))
        n_open = O.duration_mul_f32(dur, 0.5) * 11025 // NS
        ref.append(O.analyze_batch([pcm[: ch * n_open]], ch, hd)[0])
    r = subprocess.run([exe, "analyze", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for p, want in zip(paths, ref):
        rc, disk = O.frame_hashes_read(p[:-4] + ".needle.dat")
        assert rc == 0 and disk.opening == want.opening and disk.md5 == O.header_md5(p), p
    r = subprocess.run([exe, "search", str(tmp_path), "--min-opening-duration", "10"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    want = O.run_with_frame_hashes(O.Comparator(min_opening_duration=10 * NS), ref)
    found = 0
    for p, w in zip(paths, want):
        if w is not None and w.opening is not None:
            assert f'{p}\n\n* Opening - "{O.format_time(w.opening[0])}"-"{O.format_time(w.opening[1])}"' in r.stdout
            found += 1
    assert found >= 3 and r.stdout.count("* Opening") == found


@pytest.fixture(scope="module")
def lib28x6():
    """configs[1]'s shape with 6-channel audio: 28 episodes x 24 min at 11025 Hz, 90 s shared intro."""
    eps = synth.make_library(28, 24 * 60.0, 90.0)
    return [_episode6(e, k) for k, e in enumerate(eps)]


def _job(lib, cmp):
    lib.job_begin(cmp, 0)
    res, _ = lib.job_end(cmp, 0)
    runs = lib.job_runs(0)
    return res, runs


def _same(got, want):
    assert [None if r is None else (r.opening, r.ending) for r in got] == \
           [None if r is None else (r.opening, r.ending) for r in want]


def test_library_of_six_channel_episodes_at_config1_scale(lib28x6):
    """set_pcm (staged down-mix into a mono resident PCM), set_pcm_device (the caller's device pointers, 2 bytes off a
    16-byte boundary) and stream_pcm on 28 x 24 min of 6-channel PCM: job results equal the oracle's, the run lists of
    the three are the same, and the audit of the resident PCM finds no mismatch."""
    n, ch = len(lib28x6), 6
    threads = min(os.cpu_count() or 1, 16)
    hd = O.duration_from_secs_f32(0.3)
    lens = [len(p) for p in lib28x6]
    ref = O.analyze_batch([p[: ch * ((len(p) // ch) // 2)] for p in lib28x6], ch, hd, threads=threads)
    want = O.run_with_frame_hashes(O.Comparator(), ref, threads=threads)
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(n)])

    lib = capi.Library(n)
    lib.set_pcm(lib28x6, lens, channels=ch)
    got, runs = _job(lib, cmp)
    _same(got, want)
    assert sum(r is not None and r.opening is not None for r in got) == n
    for v in (0, n - 1):
        assert lib.frame_hashes(v).opening_data()[0].tolist() == [h for h, _ in ref[v].opening]
    audit = lib.audit()
    assert audit["items"] == n * 2897 and audit["mismatches"] == 0 and audit["accepted_mismatches"] == 0
    del lib

    L = capi.lib()
    bufs, ptrs = [], []
    for p in lib28x6:
        b = capi.DeviceBuffer(p.nbytes + 16)
        capi.check(L.needle_hip_memcpy_h2d(b.ptr + 2, p.ctypes.data, p.nbytes))
        bufs.append(b)
        ptrs.append(b.ptr + 2)
    dev = capi.Library(n)
    dev.set_pcm_device(ptrs, lens, channels=ch)
    del bufs                                                                   # free on return
    got_d, runs_d = _job(dev, cmp)
    _same(got_d, want)
    assert np.array_equal(np.sort(runs_d, order=["problem", "src_end", "dst_end"]),
                          np.sort(runs, order=["problem", "src_end", "dst_end"]))
    del dev

    st = capi.Library(n)
    st.stream_pcm(lib28x6, lens, channels=ch)
    got_s, runs_s = _job(st, cmp)
    _same(got_s, want)
    assert np.array_equal(np.sort(runs_s, order=["problem", "src_end", "dst_end"]),
                          np.sort(runs, order=["problem", "src_end", "dst_end"]))


def test_library_staging_in_small_groups_and_two_simulated_ranks(monkeypatch):
    """set_pcm's staging buffer cut to a few thousand values (many groups, windows in pieces), and the multi-GPU plan
    with two Library objects standing in for two ranks that each hold only their own episodes' 6-channel PCM
    (as test_two_simulated_ranks_on_one_device_equal_single_library does for mono): results equal the oracle's."""
    from tests import dist_plan as ndist
    n, world, ch = 7, 2, 6
    eps = synth.make_library(n, 90.0, 20.0)
    pcm6 = [_episode6(e, k) for k, e in enumerate(eps)]
    lens = [len(p) for p in pcm6]
    hd = O.duration_from_secs_f32(0.3)
    ref = O.analyze_batch([p[: ch * ((len(p) // ch) // 2)] for p in pcm6], ch, hd)
    want = O.run_with_frame_hashes(O.Comparator(min_opening_duration=10 * NS), ref)
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(n)], min_opening_duration=10)
    cap = 4096

    monkeypatch.setenv("NEEDLE_HIP_MAX_BATCH_VALUES", "30001")
    one = capi.Library(n)
    one.set_pcm(pcm6, lens, channels=ch)
    monkeypatch.delenv("NEEDLE_HIP_MAX_BATCH_VALUES")
    one.analyze(0, n)
    for v in range(n):
        assert one.frame_hashes(v).opening_data()[0].tolist() == [h for h, _ in ref[v].opening]

    L = capi.lib()
    b = ndist.block(n, world)
    libs, arenas = [], []
    for rank in range(world):
        first, count = ndist.shard(n, world, rank)
        lib = capi.Library(n)
        lib.set_pcm([p if first <= k < first + count else None for k, p in enumerate(pcm6)], lens, channels=ch)
        _, stride = lib.hash_arena()
        buf = capi.DeviceBuffer(b * world * stride * 4)
        zeros = np.zeros(b * world * stride, dtype=np.uint32)
        capi.check(L.needle_hip_memcpy_h2d(buf.ptr, zeros.ctypes.data, zeros.nbytes))
        lib.use_hash_arena(buf.ptr, b * world, stride)
        if count:
            lib.analyze(first, count)
        libs.append(lib)
        arenas.append(buf)
    host = [a.to_host(np.uint32, b * world * stride).reshape(b * world, stride) for a in arenas]
    full = np.zeros_like(host[0])
    for rank in range(world):
        full[rank * b:(rank + 1) * b] = host[rank][rank * b:(rank + 1) * b]
    for a in arenas:
        capi.check(L.needle_hip_memcpy_h2d(a.ptr, full.ctypes.data, full.nbytes))
    runs = []
    for rank in range(world):
        pfirst, pcount = ndist.shard(ndist.pair_count(n), world, rank)
        d_runs, d_count = capi.DeviceBuffer(cap * capi.RUN_DTYPE.itemsize), capi.DeviceBuffer(4)
        libs[rank].search(cmp, pfirst, pcount, d_runs.ptr, cap, d_count.ptr, sync=True)
        runs.append(d_runs.to_host(capi.RUN_DTYPE, int(d_count.to_host(np.uint32, 1)[0])))
    _same(libs[0].finalize(cmp, np.concatenate(runs)), want)


def test_chromaprint_compat_stays_one_or_two_channels():
    """The libchromaprint compatibility layer keeps its 1-2 channel contract (its exported-constants test pins
    start(ctx, 11025, 6) == 0); 3-8 channel callers use the needle_hip_* entry points."""
    from .test_capi_cpu import _chromaprint_lib
    L = _chromaprint_lib()
    ctx = L.chromaprint_new(1)
    assert L.chromaprint_start(ctx, 48000, 6) == 0 and L.chromaprint_start(ctx, 48000, 2) == 1
    L.chromaprint_free(ctx)
