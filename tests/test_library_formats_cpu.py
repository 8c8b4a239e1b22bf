"""A format per video in a library (needle_hip_library_set_video_formats), the part that needs no device: every refusal
of the formats, of the setters beside them and of the PCM calls' `channels` comes back as InvalidArgument before a device
is asked for (a call that gets as far as the device fails with "no HIP device" on a machine without one) and leaves the
library as it was -- all but one: that set_video_formats is refused AFTER a PCM call can only be shown where a PCM call
succeeds, so that case needs a device (here when there is one, and in tests/test_gpu_library_formats.py); rank_videos(channels=0) is host arithmetic on the
formats and the lengths; the host plan of the uploads runs under ASan/UBSan in a program of its own."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from needle_amd import capi
from tests.test_gpu_library_rates import ENDING, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, INVALID = 2, 3
STEP = 2                                                                      # 300 ms / 123 ms
SEASON = [(1, 11025, capi.SAMPLE_S16), (2, 11025, capi.SAMPLE_S16), (2, 44100, capi.SAMPLE_S16),
          (6, 48000, capi.SAMPLE_F32P), (2, 48000, capi.SAMPLE_S32), (1, 32000, capi.SAMPLE_U8P),
          (2, 22050, capi.SAMPLE_F64)]
SYMBOLS = ["needle_hip_library_set_video_formats", "needle_hip_library_video_format", "needle_hip_analyzer_run_pcm_formats"]


def season_mixes():
    return [capi.channel_mix_default(0x3F) if ch == 6 else None for ch, _, _ in SEASON]


def invalid(call, *args, **kw):
    with pytest.raises(capi.NeedleError) as e:
        call(*args, **kw)
    assert e.value.name == "InvalidArgument", e.value


def formats_of(lib):
    return [lib.video_format(v) for v in range(lib.n)]


def test_entry_points_are_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "needle_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "needle-hip", "src", "ffi.rs")).read()
    for fn in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % fn, text), fn
        assert fn in capi.NEEDLE_HIP_H_SYMBOLS and hasattr(capi.lib(), fn), fn
        assert re.search(r"pub fn %s\s*\(" % fn, ffi), fn


def test_null_arguments():
    L = capi.lib()
    lib = capi.Library(7)
    f = capi._lane_formats(SEASON)
    one = capi.CLaneFormat()
    assert L.needle_hip_library_set_video_formats(None, f, None) == NULL
    assert L.needle_hip_library_set_video_formats(lib._h, None, None) == NULL
    assert L.needle_hip_library_video_format(None, 0, C.byref(one)) == NULL
    assert L.needle_hip_library_video_format(lib._h, 0, None) == NULL
    assert L.needle_hip_library_video_format(lib._h, 0, C.byref(one)) == INVALID          # no formats yet
    lib.set_video_formats(SEASON, season_mixes())
    assert formats_of(lib) == SEASON
    assert L.needle_hip_library_video_format(lib._h, 7, C.byref(one)) == INVALID          # out of range


def test_both_kinds_of_setter_exclude_each_other():
    for setter in (lambda l: l.set_sample_rate(48000), lambda l: l.set_sample_format(capi.SAMPLE_F32),
                   lambda l: l.set_channel_mix(capi.channel_mix_default(0x3F)), lambda l: l.set_channel_mix(None)):
        lib = capi.Library(7).include_endings(ENDING)
        setter(lib)
        invalid(lib.set_video_formats, SEASON)                                           # it after them
        invalid(lib.video_format, 0)
        lib = capi.Library(7).set_video_formats(SEASON)
        invalid(setter, lib)                                                             # them after it
        assert formats_of(lib) == SEASON
    lib = capi.Library(7).set_video_formats(SEASON).include_endings(ENDING)              # include_endings on either side
    assert lib.rows_per_video() == 2 and formats_of(lib) == SEASON


@pytest.mark.parametrize("video", [0, 3, 6])
def test_a_bad_video_refuses_the_whole_array_and_changes_nothing(video):
    first = [(2, 48000, capi.SAMPLE_S16)] * 7
    lib = capi.Library(7).set_video_formats(first)

    def with_video(fmt):
        return [fmt if v == video else f for v, f in enumerate(SEASON)]
    ch, rate, fmt = SEASON[video]
    for bad in ((0, rate, fmt), (9, rate, fmt), (-1, rate, fmt), (ch, 1999, fmt), (ch, 768001, fmt), (ch, 0, fmt),
                (ch, rate, -1), (ch, rate, 10), (ch, 44101, fmt)):                       # (44101: no resampler design)
        invalid(lib.set_video_formats, with_video(bad), season_mixes())
        assert formats_of(lib) == first, bad
    wrong = season_mixes()
    wrong[video] = capi.channel_mix_default(0x60F if ch != 6 else 0x3)                   # a mix for another channel count
    invalid(lib.set_video_formats, SEASON, wrong)
    assert formats_of(lib) == first
    # the refused mixes did not stick either: the plan of the accepted array is the stereo library's
    lens = [48000 * 25 * 2] * 7
    assert lib.rank_videos(lens, 3, 1, channels=0) == \
        capi.Library(7).set_sample_rate(48000).rank_videos(lens, 3, 1, channels=2)
    lib.set_video_formats(SEASON, season_mixes())                                        # and a good array is still taken
    assert formats_of(lib) == SEASON


def test_channels_of_the_pcm_calls():
    """channels != 0 with formats and channels == 0 without are InvalidArgument from every PCM call and rank_videos, before
    a device is asked for."""
    L = capi.lib()
    frames = [rate * 20 for _, rate, _ in SEASON]
    lens = [f * ch for f, (ch, _, _) in zip(frames, SEASON)]
    pcm = [np.zeros(16, np.int16)] * 7
    with_formats = capi.Library(7).set_video_formats(SEASON)
    without = capi.Library(7)
    for lib, bad in ((with_formats, (1, 2, 6, 8, -1, 9)), (without, (0, -1, 9))):
        for ch in bad:
            sz = (C.c_size_t * 7)(*lens)
            ptrs = (C.c_void_p * 12)(*[pcm[0].ctypes.data] * 12)
            assert L.needle_hip_library_set_pcm(lib._h, ptrs, sz, ch) == INVALID, ch
            assert L.needle_hip_library_stream_pcm(lib._h, ptrs, sz, ch) == INVALID, ch
            L.needle_hip_library_set_pcm_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int]
            assert L.needle_hip_library_set_pcm_device(lib._h, ptrs, sz, ch) == INVALID, ch
            invalid(lib.rank_videos, lens, 2, 0, channels=ch)
    assert formats_of(with_formats) == SEASON
    assert with_formats.rank_videos(lens, 2, 0, channels=0)[0] == 0                     # ... and both still plan
    assert without.rank_videos(lens, 2, 0, channels=1)[0] == 0


def test_formats_come_before_the_pcm(has_gpu):
    """After a PCM call set_video_formats is InvalidArgument (needs a device to get that far)."""
    lib = capi.Library(2).set_video_formats([(1, 11025, capi.SAMPLE_S16), (2, 22050, capi.SAMPLE_F32)])
    pcm = [np.zeros(11025 * 20, np.int16), np.zeros(22050 * 20 * 2, np.float32)]
    if not has_gpu:
        with pytest.raises(capi.NeedleError) as e:
            lib.set_pcm(pcm, [len(p) for p in pcm], channels=0)
        assert e.value.name == "Unknown" and "no HIP device" in str(e.value)
        lib.set_video_formats([(1, 11025, capi.SAMPLE_S16)] * 2)                         # nothing was loaded
        return
    lib.set_pcm(pcm, [len(p) for p in pcm], channels=0)
    invalid(lib.set_video_formats, [(1, 11025, capi.SAMPLE_S16)] * 2)
    assert formats_of(lib) == [(1, 11025, capi.SAMPLE_S16), (2, 22050, capi.SAMPLE_F32)]


@pytest.mark.parametrize("endings", [False, True])
def test_rank_plan_of_a_uniform_array_is_the_setters(endings):
    rng = np.random.default_rng(17)
    for ch, rate, fmt in ((1, 11025, capi.SAMPLE_S16), (2, 48000, capi.SAMPLE_S16), (6, 48000, capi.SAMPLE_F32P)):
        frames = [int(f) for f in rng.integers(rate * 60, rate * 1500, 21)] + [0, rate * 3]
        lens = [f * ch + (k % ch) for k, f in enumerate(frames)]
        n = len(lens)
        mix = capi.channel_mix_default(0x3F) if ch == 6 else None
        a = capi.Library(n).set_sample_rate(rate).set_sample_format(fmt).set_channel_mix(mix)
        b = capi.Library(n).set_video_formats([(ch, rate, fmt)] * n, [mix] * n)
        if endings:
            a.include_endings(ENDING)
            b.include_endings(ENDING)
        for world in range(1, 9):
            for rank in range(world):
                assert b.rank_videos(lens, world, rank, channels=0) == a.rank_videos(lens, world, rank, channels=ch), \
                    (ch, world, rank)


def restated_rank_videos(lens, formats, endings, world, rank):
    """library.cpp's plan: kept hashes per row from windows() at the video's own rate, the resampler's output length
    and num_kept; the arena's stride; the rows this rank's flat block of the arena meets."""
    L = capi.lib()
    L.needle_hip_resample_out_len.restype = C.c_size_t
    L.needle_hip_resample_out_len.argtypes = [C.c_size_t, C.c_int]
    L.needle_hip_fingerprint_num_kept.restype = C.c_size_t
    L.needle_hip_fingerprint_num_kept.argtypes = [C.c_size_t, C.c_uint32]
    R = 2 if endings else 1
    kept = []
    for n_values, (ch, rate, _) in zip(lens, formats):
        (_, n_open), (_, n_end, _) = windows(n_values, ch, rate)
        for count in (n_open, n_end)[:R]:
            kept.append(L.needle_hip_fingerprint_num_kept(L.needle_hip_resample_out_len(int(count), rate), STEP))
    n, rows = len(lens), len(kept)
    if world == 1:
        return 0, n
    tiles = max(1, (max(kept) + 63) // 64)
    while rows * tiles % world:
        tiles += 1
    stride = 64 * tiles
    block = rows * stride // world
    begin, end = rank * block, (rank + 1) * block
    videos = [row // R for row in range(rows)
              if max(begin - row * stride, 0) < min(end - row * stride, stride, kept[row])]
    return (videos[0], videos[-1] - videos[0] + 1) if videos else (0, 0)


@pytest.mark.parametrize("endings", [False, True])
def test_rank_plan_of_a_mixed_array(endings):
    rng = np.random.default_rng(23)
    formats = [SEASON[k % 7] for k in range(23)]
    frames = [int(rng.integers(rate * 60, rate * 1500)) for _, rate, _ in formats]
    frames[5], frames[11] = 0, formats[11][1] * 3
    lens = [f * ch + (k % ch) for k, (f, (ch, _, _)) in enumerate(zip(frames, formats))]
    lib = capi.Library(len(lens)).set_video_formats(formats)
    if endings:
        lib.include_endings(ENDING)
    seen = set()
    for world in range(1, 9):
        for rank in range(world):
            got = lib.rank_videos(lens, world, rank, channels=0)
            assert got == restated_rank_videos(lens, formats, endings, world, rank), (world, rank)
            seen.add(got)
    assert len(seen) > 20                                                               # (the plans do differ)


def test_analyzer_refusals():
    L = capi.lib()
    an = capi.Analyzer.from_files(["a.wav", "b.wav"])
    h = an._handle()
    x = np.zeros(64, np.float32)
    n = (C.c_size_t * 2)(64, 64)
    p = (C.c_void_p * 3)(x.ctypes.data, x.ctypes.data, x.ctypes.data)
    f = capi._lane_formats([(1, 11025, capi.SAMPLE_F32), (2, 48000, capi.SAMPLE_F32P)])
    assert L.needle_hip_analyzer_run_pcm_formats(None, p, n, f, None, 0.3, False) == NULL
    assert L.needle_hip_analyzer_run_pcm_formats(h, None, n, f, None, 0.3, False) == NULL
    assert L.needle_hip_analyzer_run_pcm_formats(h, p, None, f, None, 0.3, False) == NULL
    assert L.needle_hip_analyzer_run_pcm_formats(h, p, n, None, None, 0.3, False) == NULL
    assert L.needle_hip_analyzer_run_pcm_formats(h, p, n, f, None, 0.0, False) == 9     # AnalyzerInvalidHashDuration
    half = (C.c_void_p * 3)(x.ctypes.data, x.ctypes.data, None)
    assert L.needle_hip_analyzer_run_pcm_formats(h, half, n, f, None, 0.3, False) == NULL
    for bad in ((0, 11025, capi.SAMPLE_F32), (9, 11025, capi.SAMPLE_F32), (1, 1999, capi.SAMPLE_F32),
                (1, 768001, capi.SAMPLE_F32), (1, 11025, 10), (1, 11025, -1), (1, 44101, capi.SAMPLE_F32)):
        g = capi._lane_formats([bad, (2, 48000, capi.SAMPLE_F32P)])
        assert L.needle_hip_analyzer_run_pcm_formats(h, p, n, g, None, 0.3, False) == INVALID, bad
    wrong = capi._channel_mixes([None, capi.channel_mix_default(0x3F)])                  # a 6-channel mix on a stereo stream
    assert L.needle_hip_analyzer_run_pcm_formats(h, p, n, f, wrong, 0.3, False) == INVALID
    mixed = capi.Analyzer.from_files(["a.wav", "b.wav"]).set_channel_mix(capi.channel_mix_default(0x3))
    invalid(mixed.run_pcm_formats, [x, [x[:32], x[32:]]], [(1, 11025, capi.SAMPLE_F32), (2, 48000, capi.SAMPLE_F32P)],
            [None, capi.channel_mix_default(0x3)])                                      # both kinds of mix in one call


def test_host_plan_under_address_and_ub_sanitizers():
    """tests/cpp/format_plan_check.cpp: piece cutting per rate and the pointer-array walk with planar and NULL videos, in
    a program of its own built with -fsanitize=address,undefined."""
    gcc = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True)
    if gcc.returncode != 0 or not os.path.isabs(gcc.stdout.strip()) or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no libasan / hipcc here")
    csrc = os.path.join(ROOT, "needle_amd", "csrc")
    subprocess.run(["make", "-s", "-j", "8", "-C", csrc, "all"], check=True)
    subprocess.run(["make", "-s", "-j", "8", "-C", csrc, "../../build/asan/format_plan_check"], check=True)
    out = subprocess.run([os.path.join(ROOT, "build", "asan", "format_plan_check")], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0 and "format plan ok" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "runtime error:" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
