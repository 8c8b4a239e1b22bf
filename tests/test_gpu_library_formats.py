"""A rate, channel count, sample format and mix per video in one library and in one analyzer call, on the MI355X
(needle_hip_library_set_video_formats, needle_hip_analyzer_run_pcm_formats).  One season of seven videos of 22 to 30 s
with a planted opening and ending, each rendered into a format of its own, goes through set_pcm, set_pcm_device and
stream_pcm, whole and in pieces, on one rank and on two simulated ones.  The expected values are always the oracle's: a
window cut at the video's own rate, the numpy statement of the conversion (tests/test_sample_formats_cpu.py), the
oracle's plain average or the mix of tests/channel_mix.py, oracle.resample, oracle.fingerprint, the oracle's comparator.
Every comparison is bit-exact.

The season is the issue's table with two rates swapped so that the rates cover every resampler family
needle_hip_resample_plan distinguishes: video 5 is at 96000 Hz (DPP quads) instead of 48000, video 7 at 9000 Hz (the
general kernel) instead of 22050; 44100 Hz is an integer decimation, 48000 and 32000 Hz run on the matrix cores."""
import struct

import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests import channel_mix as M
from tests.pipeline_worker import sorted_runs
from tests.test_gpu_library_rates import ENDING, at_rate, hashes_of, job, oracle_hashes, results
from tests.test_gpu_scan_threshold import _min_len_for
from tests.test_gpu_sample_formats import in_format, oracle_frame_hashes, stream_of
from tests.test_sample_formats_cpu import to_s16

pytestmark = pytest.mark.gpu
NS = O.NS
MASK_51 = 0x3F
# channels, rate, format, channel mask of the mix (None: the plain average), seconds
SEASON = [(1, 11025, capi.SAMPLE_S16, None, 24), (2, 11025, capi.SAMPLE_S16, None, 22), (2, 44100, capi.SAMPLE_S16, None, 27),
          (6, 48000, capi.SAMPLE_F32P, MASK_51, 23), (2, 96000, capi.SAMPLE_S32, None, 30), (1, 32000, capi.SAMPLE_U8P, None, 25),
          (2, 9000, capi.SAMPLE_F64, None, 26)]
FORMATS = [(ch, rate, fmt) for ch, rate, fmt, _, _ in SEASON]
RATES = sorted({rate for _, rate, _ in FORMATS} - {11025})
INTRO, OUTRO = 8.0, 5.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def test_the_rates_cover_every_resampler_family():
    families = {capi.resample_plan(rate)["family"] for _, rate, _ in FORMATS}
    assert families == {"identity", "dec", "mfma", "quad", "general"}, families


def mixes(season=SEASON):
    return [None if s[3] is None else capi.channel_mix_default(s[3]) for s in season]


def oracle_video(raw, ch, rate, fmt, mask, endings=True):
    """The oracle's FrameHashes of one video: conversion, then the plain average (the oracle's own, in its resampler or
    its fingerprinter) or the mix, the windows cut at the video's rate."""
    s16 = to_s16(raw, fmt)
    if mask is None:
        return oracle_frame_hashes(s16, ch, rate, endings)
    return oracle_frame_hashes(M.fold_mono(s16, *M.default_rows(mask)), 1, rate, endings)


class Season:
    def __init__(self, season=SEASON, seed=0):
        self.season = season
        self.n = len(season)
        self.formats = [(ch, rate, fmt) for ch, rate, fmt, _, _ in season]
        self.raw, self.streams = [], []
        for k, (ch, rate, fmt, mask, seconds) in enumerate(season):
            mono = synth.make_episode(k, float(seconds), INTRO, OUTRO).pcm
            x = in_format(at_rate(mono, rate, ch, k + seed), fmt, 40 + k)
            self.raw.append(x)
            self.streams.append(stream_of(x, ch, fmt))
        self.lens = [len(x) for x in self.raw]
        self.ref = [oracle_video(x, ch, rate, fmt, mask) for x, (ch, rate, fmt, mask, _) in zip(self.raw, season)]
        self.names = [f"ep{k}.wav" for k in range(self.n)]

    def library(self, endings=True):
        lib = capi.Library(self.n)
        if endings:
            lib.include_endings(ENDING)
        return lib.set_video_formats(self.formats, mixes(self.season))

    def device_copies(self, held=None):
        """Every plane in a device buffer of its own, one sample past a 16-byte boundary; None for the planes of videos
        that are not `held`."""
        L = capi.lib()
        bufs, ptrs = [], []
        for v, (stream, (ch, _, fmt)) in enumerate(zip(self.streams, self.formats)):
            planes = stream if capi.sample_format_planar(fmt) else [stream]
            for p in planes:
                if held is not None and v not in held:
                    ptrs.append(None)
                    continue
                b = capi.DeviceBuffer(p.nbytes + 32)
                at = (b.ptr + 15) // 16 * 16 + p.itemsize
                capi.check(L.needle_hip_memcpy_h2d(at, p.ctypes.data, p.nbytes))
                bufs.append(b)
                ptrs.append(at)
        return bufs, ptrs


@pytest.fixture(scope="module")
def season():
    return Season()


@pytest.fixture(scope="module")
def expected(season):
    """(the oracle's results, the Comparator that asks for them)"""
    want = O.run_with_frame_hashes(O.Comparator(include_endings=True, min_opening_duration=5 * NS, min_ending_duration=3 * NS),
                                   season.ref)
    assert sum(w is not None and w.opening is not None for w in want) >= 4
    assert sum(w is not None and w.ending is not None for w in want) >= 3
    cmp = capi.Comparator(season.names, include_endings=True, min_opening_duration=5, min_ending_duration=3)
    return want, cmp


def load(season, lib, door, held=None):
    pcm = [s if held is None or v in held else None for v, s in enumerate(season.streams)]
    if door == "set_pcm":
        lib.set_pcm(pcm, season.lens, channels=0)
    elif door == "stream_pcm":
        lib.stream_pcm(pcm, season.lens, channels=0)
    else:
        bufs, ptrs = season.device_copies(held)
        lib.set_pcm_device(ptrs, season.lens, channels=0)
        del bufs                                                                   # the caller's buffers are free on return


def check_library(season, lib, expected, runs_like=None):
    want, cmp = expected
    got, runs = job(lib, cmp)
    assert results(got) == results(want)
    for v in range(season.n):
        assert hashes_of(lib.frame_hashes(v)) == oracle_hashes(season.ref[v]), v
    if runs_like is not None:
        assert np.array_equal(sorted_runs(runs), runs_like)
    return runs


@pytest.fixture(scope="module")
def oracle_runs(season):
    """The oracle's sorted run list [k, 6] of the season, as tests/test_gpu_pipeline.py states it: the table-free scan
    pair by pair and region by region (problem = pair * 2 + region), each pair at the larger of its two rows' minimum
    run lengths, with the simhashes of both ends."""
    rows = [[[h for h, _ in reg] for reg in (f.opening, f.ending)] for f in season.ref]
    ts = [[[t for _, t in reg] for reg in (f.opening, f.ending)] for f in season.ref]
    out, p = [], 0
    for i in range(season.n):
        for j in range(i + 1, season.n):
            for r, min_ns in enumerate((5 * NS, 3 * NS)):
                a, b = (_min_len_for(ts[v][r], min_ns) for v in (i, j))
                if a and b:
                    src, dst = (np.array(rows[v][r], dtype=np.uint32) for v in (i, j))
                    total, runs = O.diagonal_runs_all_pairs([src, dst], 10, max(a, b), capacity=1 << 14)
                    assert total <= len(runs)
                    for _, i_end, j_end, ln in runs.tolist():
                        out.append((p * 2 + r, i_end, j_end, ln, O.simhash32(rows[i][r][i_end - ln:i_end + 1]),
                                    O.simhash32(rows[j][r][j_end - ln:j_end + 1])))
            p += 1
    keys = np.array(out, dtype=np.int64).reshape(-1, 6)
    assert len(keys) >= 6
    return keys[np.lexsort(keys.T[::-1])]


@pytest.mark.parametrize("door", ["set_pcm", "set_pcm_device", "stream_pcm"])
def test_every_door_equals_the_oracle(season, expected, oracle_runs, door):
    lib = season.library()
    load(season, lib, door)
    check_library(season, lib, expected, oracle_runs)
    assert [lib.video_format(v) for v in range(season.n)] == season.formats


def one_tile_per_piece(limit, from_host):
    """Does a staging limit of `limit` values leave one output tile per piece for every resampled video of the season?"""
    for ch, rate, _ in FORMATS:
        if rate == 11025:
            continue
        p = capi.resample_plan(rate)
        tile_in = p["tile_outputs"] * p["M"] // p["L"] + 2 * (p["T"] // 2) + 16
        if limit // 4 // ((ch if from_host else 0) + 1) > tile_in:                # (a piece gets a quarter of the batch)
            return False
    return True


@pytest.mark.parametrize("limit", [400003, 3001, 1000])
@pytest.mark.parametrize("door", ["set_pcm", "set_pcm_device", "stream_pcm"])
def test_in_pieces(season, expected, oracle_runs, monkeypatch, door, limit):
    """A staging buffer of 3001 values, as tests/test_gpu_library_rates.py's test_windows_resampled_in_pieces chooses it:
    every window is cut into many pieces (stream_pcm: every window is a batch of its own).  3001 and 1000 values leave one
    output tile per piece at every rate of the season, 1000 also cuts the 11025 Hz windows into 16-frame groups by the
    hundred; 400003 values leave several tiles per piece and several pieces per window.  A piece takes a quarter of the
    staging at most, so batches hold pieces of different windows and formats (tests/cpp/format_plan_check.cpp counts them)."""
    assert all(one_tile_per_piece(small, host) for small in (3001, 1000) for host in (True, False))
    assert not one_tile_per_piece(400003, True) and not one_tile_per_piece(400003, False)
    monkeypatch.setenv("NEEDLE_HIP_MAX_BATCH_VALUES", str(limit))
    lib = season.library()
    load(season, lib, door)
    check_library(season, lib, expected, oracle_runs)


def arena_rows(lib, n_rows):
    arena, stride = lib.hash_arena()
    rows = np.zeros(n_rows * stride, dtype=np.uint32)
    capi.check(capi.lib().needle_hip_memcpy_d2h(rows.ctypes.data, arena, rows.nbytes))
    return rows.reshape(n_rows, stride)


@pytest.mark.parametrize("ch,rate,fmt,mask", [(2, 48000, capi.SAMPLE_S16, None), (6, 48000, capi.SAMPLE_F32P, MASK_51)])
def test_a_uniform_array_equals_the_setters(ch, rate, fmt, mask):
    n = 4
    eps = synth.make_library(n, 24.0, INTRO, outro_s=OUTRO)
    raw = [in_format(at_rate(e.pcm, rate, ch, k), fmt, 60 + k) for k, e in enumerate(eps)]
    streams = [stream_of(x, ch, fmt) for x in raw]
    lens = [len(x) for x in raw]
    mix = None if mask is None else capi.channel_mix_default(mask)
    a = capi.Library(n).include_endings(ENDING).set_sample_rate(rate).set_sample_format(fmt).set_channel_mix(mix)
    a.set_pcm(streams, lens, channels=ch)
    a.analyze(0, n)
    b = capi.Library(n).include_endings(ENDING).set_video_formats([(ch, rate, fmt)] * n, [mix] * n)
    b.set_pcm(streams, lens, channels=0)
    b.analyze(0, n)
    rows_a, rows_b = arena_rows(a, 2 * n), arena_rows(b, 2 * n)
    assert rows_a.shape == rows_b.shape and rows_a.any(axis=1).all()
    assert np.array_equal(rows_a, rows_b)


def launches_of(call):
    capi.set_kernel_timing("all,sum")
    try:
        call()
        return {k: capi.kernel_launches(k) for k in ("ingest", "rematrix", "resample", "convert", "downmix")}
    finally:
        capi.set_kernel_timing(None)


def test_launch_counts(season):
    """One set_pcm that fits one batch: ONE landing launch whatever the mixture -- "ingest" without mixes, "rematrix" with
    one -- and one resampler launch per distinct rate other than 11025 Hz.  A library without formats launches what it
    always did: the conversion kernel once and the resampler once for planar-float 5.1 at 48 kHz."""
    with_mix = season.library()
    got = launches_of(lambda: load(season, with_mix, "set_pcm"))
    assert got == {"ingest": 0, "rematrix": 1, "resample": len(RATES), "convert": 0, "downmix": 0}, got
    plain = capi.Library(season.n).include_endings(ENDING).set_video_formats(season.formats)
    got = launches_of(lambda: load(season, plain, "set_pcm"))
    assert got == {"ingest": 1, "rematrix": 0, "resample": len(RATES), "convert": 0, "downmix": 0}, got
    dev = season.library()
    got = launches_of(lambda: load(season, dev, "set_pcm_device"))
    assert got == {"ingest": 0, "rematrix": 1, "resample": len(RATES), "convert": 0, "downmix": 0}, got
    streamed = season.library()
    got = launches_of(lambda: load(season, streamed, "stream_pcm"))                  # (28 MB: one launch group)
    assert got == {"ingest": 0, "rematrix": 1, "resample": len(RATES), "convert": 0, "downmix": 0}, got
    ch, rate, fmt = FORMATS[3]
    uniform = capi.Library(2).include_endings(ENDING).set_sample_rate(rate).set_sample_format(fmt)
    got = launches_of(lambda: uniform.set_pcm([season.streams[3]] * 2, [season.lens[3]] * 2, channels=ch))
    assert got == {"ingest": 0, "rematrix": 0, "resample": 1, "convert": 1, "downmix": 0}, got
    stereo = capi.Library(2).include_endings(ENDING)
    got = launches_of(lambda: stereo.set_pcm([season.streams[1]] * 2, [season.lens[1]] * 2, channels=2))
    assert got == {"ingest": 0, "rematrix": 0, "resample": 0, "convert": 0, "downmix": 0}, got


def test_surround_with_its_default_mix_hashes_like_its_fold_down(season):
    """Within one library: the 5.1 video under the default mix of its mask, and a stereo s16 video holding the fold-down
    (Lo, Ro) of tests/channel_mix.py, hash bit for bit alike."""
    ch, rate, fmt = FORMATS[3]
    lo, ro = M.fold_stereo(to_s16(season.raw[3], fmt), *M.default_rows(MASK_51))
    stereo = M.interleave(lo, ro)
    lib = capi.Library(2).include_endings(ENDING).set_video_formats([(ch, rate, fmt), (2, rate, capi.SAMPLE_S16)],
                                                                     [capi.channel_mix_default(MASK_51), None])
    lib.set_pcm([season.streams[3], stereo], [season.lens[3], len(stereo)], channels=0)
    lib.analyze(0, 2)
    assert hashes_of(lib.frame_hashes(0)) == hashes_of(lib.frame_hashes(1)) == oracle_hashes(season.ref[3])
    assert len(season.ref[3].opening) > 20 and len(season.ref[3].ending) > 10


def test_two_simulated_ranks(season):
    """rank_videos(channels=0) picks each rank's videos; two Library objects standing in for two ranks are given only
    those (NULL planes elsewhere) and fingerprint them; their rows together give the oracle's hashes and results."""
    n, world = season.n, 2
    ref = [oracle_video(x, ch, rate, fmt, mask, endings=False) for x, (ch, rate, fmt, mask, _) in zip(season.raw, SEASON)]
    for f in ref:
        f.ending = []
    want = O.run_with_frame_hashes(O.Comparator(min_opening_duration=5 * NS), ref)
    single = season.library(endings=False)
    load(season, single, "set_pcm")
    cmp = capi.Comparator(season.names, min_opening_duration=5)
    got_single, _ = job(single, cmp)
    L = capi.lib()
    plans = [season.library(endings=False).rank_videos(season.lens, world, r, channels=0) for r in range(world)]
    assert plans[0][0] == 0 and plans[-1][0] + plans[-1][1] == n and all(c > 0 for _, c in plans)
    libs = []
    for r, (first, count) in enumerate(plans):
        lib = season.library(endings=False)
        load(season, lib, "set_pcm" if r == 0 else "set_pcm_device", held=set(range(first, first + count)))
        lib.analyze(first, count)
        libs.append(lib)
    stride = libs[0].hash_arena()[1]
    full = np.zeros((n, stride), dtype=np.uint32)
    for lib, (first, count) in zip(libs, plans):
        full[first:first + count] = arena_rows(lib, n)[first:first + count]
    for v in range(n):
        assert full[v][: len(ref[v].opening)].tolist() == [h for h, _ in ref[v].opening], v
    capi.check(L.needle_hip_memcpy_h2d(libs[0].hash_arena()[0], full.ctypes.data, full.nbytes))
    cap = 4096
    d_runs, d_count = capi.DeviceBuffer(cap * capi.RUN_DTYPE.itemsize), capi.DeviceBuffer(4)
    libs[0].search(cmp, 0, libs[0].num_pairs(), d_runs.ptr, cap, d_count.ptr, sync=True)
    runs = d_runs.to_host(capi.RUN_DTYPE, int(d_count.to_host(np.uint32, 1)[0]))
    assert results(libs[0].finalize(cmp, runs)) == results(want) == results(got_single)


def test_audit_after_a_job(season, expected):
    lib = season.library()
    load(season, lib, "set_pcm")
    check_library(season, lib, expected)
    audit = lib.audit()
    assert audit["mismatches"] == 0 and audit["accepted_mismatches"] == 0
    assert audit["items"] == sum(len(f.opening) + len(f.ending) for f in season.ref)


def test_analyzer_run_pcm_formats_equals_the_oracle(season, expected):
    want, cmp = expected
    an = capi.Analyzer.from_files(season.names).with_include_endings(True).with_ending_search_percentage(ENDING)
    fhs = an.run_pcm_formats(season.streams, season.formats, mixes())
    for v in range(season.n):
        assert hashes_of(fhs[v]) == oracle_hashes(season.ref[v]), v
    assert results(cmp.run_with_frame_hashes(fhs)) == results(want)
    # per video it is run_pcm_format's result for that video alone (the 5.1 one with its mix on the analyzer)
    for v in (3, 6):
        ch, rate, fmt = season.formats[v]
        alone = capi.Analyzer.from_files([season.names[v]]).with_include_endings(True).with_ending_search_percentage(ENDING)
        alone.set_channel_mix(mixes()[v])
        assert hashes_of(alone.run_pcm([season.streams[v]], channels=ch, sample_rate=rate, sample_format=fmt)[0]) == \
            hashes_of(fhs[v]), v


def test_a_refused_pcm_call_leaves_the_library_as_it_was(season, expected, oracle_runs):
    lib = season.library()
    load(season, lib, "set_pcm")
    check_library(season, lib, expected, oracle_runs)
    half = list(season.streams)
    half[3] = list(half[3])
    keep, flat, _ = capi._lane_pointers(half, season.formats)
    flat[5] = None                                                                   # one plane of the 5.1 video is missing
    ptrs = (capi.C.c_void_p * len(flat))(*flat)
    lens = (capi.C.c_size_t * season.n)(*season.lens)
    L = capi.lib()
    assert L.needle_hip_library_set_pcm(lib._h, ptrs, lens, 0) == 2                  # NullArgument
    assert L.needle_hip_library_stream_pcm(lib._h, ptrs, lens, 0) == 2
    for door in (lib.set_pcm, lib.stream_pcm):
        with pytest.raises(capi.NeedleError) as e:
            door(season.streams, season.lens, channels=2)
        assert e.value.name == "InvalidArgument"
    with pytest.raises(capi.NeedleError):
        lib.set_video_formats(season.formats)                                        # after the PCM: refused
    check_library(season, lib, expected, oracle_runs)
    audit = lib.audit()                                                              # the resident PCM is still the season's
    assert audit["mismatches"] == 0 and audit["items"] == sum(len(f.opening) + len(f.ending) for f in season.ref)


def write_wav(path, x, channels, rate, tag, bits, mask=None):
    """Interleaved samples as RIFF/WAVE: tag 1 (integer PCM) or 3 (IEEE float); with a mask, WAVE_FORMAT_EXTENSIBLE
    carrying dwChannelMask and the tag as its sub-format."""
    payload = np.ascontiguousarray(x).tobytes()
    align = channels * bits // 8
    fmt = struct.pack("<HHIIHH", tag if mask is None else 0xFFFE, channels, rate, rate * align, align, bits)
    if mask is not None:
        fmt += struct.pack("<HHI", 22, bits, mask) + struct.pack("<IHH", tag, 0, 0x10) + bytes([0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71])
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(payload)) + payload
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_a_directory_of_wav_files_in_one_pass(season, tmp_path, monkeypatch, capfd):
    """Five WAV files in formats of their own -- s16 mono 11025 Hz, s16 stereo 44.1 kHz, s32 stereo 96 kHz, f64 stereo 9 kHz and
    the f32 5.1 one with its channel mask -- through needle_audio_analyzer_run with the layout down-mix: the .needle.dat
    files are byte for byte the oracle's writer's, after ONE "read + upload + fingerprint" pass."""
    videos = [0, 2, 3, 4, 6]
    encodings = {capi.SAMPLE_S16: (1, 16), capi.SAMPLE_S32: (1, 32), capi.SAMPLE_F32P: (3, 32), capi.SAMPLE_F64: (3, 64)}
    paths = []
    for v in videos:
        ch, rate, fmt, mask, _ = SEASON[v]
        paths.append(str(tmp_path / f"ep{v}.wav"))
        write_wav(paths[-1], season.raw[v], ch, rate, *encodings[fmt], mask=mask)
    monkeypatch.setenv("NEEDLE_HIP_TRACE", "1")
    capfd.readouterr()
    an = (capi.Analyzer.from_files(paths, force=True).with_include_endings(True).with_ending_search_percentage(ENDING)
          .set_layout_downmix(True))
    got = an.run(persist=True)
    trace = capfd.readouterr().err
    assert trace.count("analyzer read + upload + fingerprint") == 1, trace
    for p, v, g in zip(paths, videos, got):
        assert hashes_of(g) == oracle_hashes(season.ref[v]), v
        want = O.FrameHashes(season.ref[v].opening, season.ref[v].ending, season.ref[v].hash_duration, O.header_md5(p))
        assert O.frame_hashes_write(str(tmp_path / "want.dat"), want) == 0
        assert open(p[:-4] + ".needle.dat", "rb").read() == open(tmp_path / "want.dat", "rb").read(), v
    # files that share one key keep the pass per key they always had
    capfd.readouterr()
    capi.Analyzer.from_files(paths[:1] * 2, force=True).run()
    assert capfd.readouterr().err.count("analyzer read + upload + fingerprint") == 1
