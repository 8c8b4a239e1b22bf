"""PCM in the decoder's sample format, at the host boundary and without a GPU: the enum and the three entry points are
declared, exported and mirrored in the Python and Rust bindings; the library setter validates its argument; the
multi-GPU plan does not depend on the format; and the compute calls fail loudly where there is no device.

The numpy statement of the conversion (include/needle_hip.h, "sample formats"; hostutil.cpp wav_convert) lives here:
`to_s16` for one array of samples, `convert_spec` for a stream.  tests/test_gpu_sample_formats.py imports both."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from needle_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORMAT_NAMES = ["U8", "S16", "S32", "F32", "F64", "U8P", "S16P", "S32P", "F32P", "F64P"]


def to_s16(x, sample_format):
    """One sample -> s16, elementwise.  U8: (x - 128) << 8.  S16: x.  S32: x >> 16 (arithmetic).  F32: rint(x * 32768)
    in f32, ties to even, NaN -> 0, otherwise clipped to [-32768, 32767].  F64: the same in f64."""
    base = sample_format % 5
    dtype = capi.sample_format_dtype(sample_format)
    x = np.asarray(x, dtype=dtype)
    if base == capi.SAMPLE_U8:
        return ((x.astype(np.int32) - 128) << 8).astype(np.int16)
    if base == capi.SAMPLE_S16:
        return x.copy()
    if base == capi.SAMPLE_S32:
        return (x >> 16).astype(np.int16)
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.rint(x * dtype.type(32768.0))                      # stays in x's precision
        assert y.dtype == dtype
        return np.where(np.isnan(y), 0, np.clip(y, -32768, 32767)).astype(np.int16)


def convert_spec(stream, channels, sample_format, num_values=None):
    """A stream -> interleaved `channels`-channel s16.  Interleaved: one array, a trailing partial frame dropped.
    Planar: `channels` planes of num_values // channels samples each."""
    if capi.sample_format_planar(sample_format):
        frames = (sum(len(p) for p in stream) if num_values is None else num_values) // channels
        planes = [to_s16(np.asarray(p)[:frames], sample_format) for p in stream]
        return np.stack(planes, axis=1).reshape(-1) if frames else np.zeros(0, np.int16)
    n = (len(stream) if num_values is None else num_values) // channels * channels
    return to_s16(np.asarray(stream)[:n], sample_format)


def test_numpy_spec_on_the_pinned_values():
    f = np.float32
    assert to_s16(np.array([0.5, 1.5, 2.5, -0.5], f) / f(32768), capi.SAMPLE_F32).tolist() == [0, 2, 2, 0]
    assert to_s16(np.array([1.0, -1.0, 32767.5 / 32768], np.float64), capi.SAMPLE_F64).tolist() == [32767, -32768, 32767]
    assert to_s16(np.array([np.inf, -np.inf, 1e30, np.nan, 1e-40], f), capi.SAMPLE_F32).tolist() == [32767, -32768, 32767, 0, 0]
    x = (0.5 + 2.0 ** -30) / 32768
    assert to_s16(np.array([x]), capi.SAMPLE_F64).tolist() == [1]
    assert to_s16(np.array([x]).astype(f), capi.SAMPLE_F32).tolist() == [0]          # narrowed first: the tie rounds down
    s32 = np.array([-2 ** 31, 2 ** 31 - 1, 65535, -1, -65537], np.int32)
    assert to_s16(s32, capi.SAMPLE_S32P).tolist() == [-32768, 32767, 0, -1, -2]
    assert to_s16(np.array([0, 128, 255], np.uint8), capi.SAMPLE_U8).tolist() == [-32768, 0, 32512]
    planes = [np.array([1, 2, 3], np.int16), np.array([4, 5, 6], np.int16)]
    assert convert_spec(planes, 2, capi.SAMPLE_S16P).tolist() == [1, 4, 2, 5, 3, 6]
    assert convert_spec(np.arange(7, dtype=np.int32) << 16, 3, capi.SAMPLE_S32).tolist() == [0, 1, 2, 3, 4, 5]


def test_enum_and_entry_points_are_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "needle_hip.h")).read()
    for value, name in enumerate(FORMAT_NAMES):
        assert re.search(r"\bNEEDLE_HIP_SAMPLE_%s\s*=\s*%d\b" % (name, value), text), name
        assert getattr(capi, "SAMPLE_" + name) == value
    ffi = open(os.path.join(ROOT, "rust", "needle-hip", "src", "ffi.rs")).read()
    rust = open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")).read()
    L = capi.lib()
    for fn in ("needle_hip_convert_host", "needle_hip_analyzer_run_pcm_format", "needle_hip_library_set_sample_format"):
        assert re.search(r"\b%s\s*\(" % fn, text), fn
        assert fn in capi.NEEDLE_HIP_H_SYMBOLS and hasattr(L, fn), fn
        assert "pub fn %s(" % fn in ffi, fn
        assert "ffi::%s(" % fn in rust, fn
    for name, value in zip(FORMAT_NAMES, range(10)):
        assert re.search(r"\b%s = %d,\n" % (name, value), rust), name
    assert [capi.sample_format_dtype(f).itemsize for f in range(10)] == [1, 2, 4, 4, 8] * 2
    with pytest.raises(ValueError):
        capi.sample_format_dtype(10)


def test_set_sample_format_validates_its_arguments():
    L = capi.lib()
    assert L.needle_hip_library_set_sample_format(None, capi.SAMPLE_F32) == 2                  # NullArgument
    for fmt in range(10):
        lib = capi.Library(3)
        assert L.needle_hip_library_set_sample_format(lib._h, fmt) == 0
    lib = capi.Library(3)
    for bad in (-1, 10, 12):
        assert L.needle_hip_library_set_sample_format(lib._h, bad) == 3                        # InvalidArgument
        with pytest.raises(capi.NeedleError) as e:
            lib.set_sample_format(bad)
        assert e.value.name == "InvalidArgument"
    chained = capi.Library(3).set_sample_rate(48000).set_sample_format(capi.SAMPLE_F32P).include_endings(0.25)
    assert isinstance(chained, capi.Library) and chained.rows_per_video() == 2


@pytest.mark.parametrize("endings", [False, True])
def test_rank_plan_does_not_depend_on_the_format(endings):
    """needle_hip_library_rank_videos counts frames: for every format, every world size from 1 to 8 and every rank the
    plan is the plain library's."""
    rng = np.random.default_rng(11)
    for ch, rate in ((1, 11025), (2, 44100), (6, 48000)):
        frames = [int(f) for f in rng.integers(rate * 60, rate * 1500, 21)] + [0, rate * 3]
        lens = [f * ch + (k % ch) for k, f in enumerate(frames)]

        def library(fmt):
            lib = capi.Library(len(frames)).set_sample_rate(rate)
            if fmt is not None:
                lib.set_sample_format(fmt)
            return lib.include_endings(0.25) if endings else lib
        plain = library(None)
        others = [library(fmt) for fmt in range(10)]
        for world in range(1, 9):
            for rank in range(world):
                want = plain.rank_videos(lens, world, rank, channels=ch)
                for fmt, lib in enumerate(others):
                    assert lib.rank_videos(lens, world, rank, channels=ch) == want, (ch, world, rank, fmt)


def test_argument_errors_of_the_new_entry_points():
    L = capi.lib()
    n = (C.c_size_t * 1)(8)
    x = np.zeros(8, np.float32)
    out = np.zeros(8, np.int16)
    p, o = (C.c_void_p * 1)(x.ctypes.data), (C.c_void_p * 1)(out.ctypes.data)
    assert L.needle_hip_convert_host(None, n, 1, 1, capi.SAMPLE_F32, o) == 2
    assert L.needle_hip_convert_host(p, None, 1, 1, capi.SAMPLE_F32, o) == 2
    assert L.needle_hip_convert_host(p, n, 1, 1, capi.SAMPLE_F32, None) == 2
    for fmt in (-1, 10, 12):
        assert L.needle_hip_convert_host(p, n, 1, 1, fmt, o) == 3
    for ch in (0, 9):
        assert L.needle_hip_convert_host(p, n, 1, ch, capi.SAMPLE_F32, o) == 3
    an = capi.Analyzer.from_files(["a.wav"])
    h = an._handle()
    assert L.needle_hip_analyzer_run_pcm_format(None, p, n, 1, 11025, capi.SAMPLE_F32, 0.3, False) == 2
    assert L.needle_hip_analyzer_run_pcm_format(h, None, n, 1, 11025, capi.SAMPLE_F32, 0.3, False) == 2
    assert L.needle_hip_analyzer_run_pcm_format(h, p, n, 1, 11025, 10, 0.3, False) == 3
    assert L.needle_hip_analyzer_run_pcm_format(h, p, n, 1, 11025, capi.SAMPLE_F32, 0.0, False) == 9
    null_plane = (C.c_void_p * 2)(x.ctypes.data, None)                    # planar stereo with one plane missing
    assert L.needle_hip_analyzer_run_pcm_format(h, null_plane, n, 2, 11025, capi.SAMPLE_F32P, 0.3, False) == 2


def test_compute_calls_need_a_device(has_gpu):
    """There is no CPU path: without a HIP device convert, run_pcm with a format and a library's set_pcm / stream_pcm with
    a format return an error (and do not crash).  With one, the same tiny calls succeed."""
    x = (np.arange(-40000, 40000, dtype=np.float32) / np.float32(32768.0))
    planes = [x[: 30000], x[30000: 60000]]

    def calls():
        yield lambda: capi.convert([x], 1, capi.SAMPLE_F32)
        yield lambda: capi.convert([planes], 2, capi.SAMPLE_F32P)
        yield lambda: capi.Analyzer.from_files(["a.wav"]).run_pcm([planes], channels=2, sample_format=capi.SAMPLE_F32P)
        yield lambda: capi.Analyzer.from_files(["a.wav"]).run_pcm([x.astype(np.float64)], sample_format=capi.SAMPLE_F64)
        yield lambda: capi.Library(1).set_sample_format(capi.SAMPLE_F32).set_pcm([x], [len(x)])
        yield lambda: capi.Library(1).set_sample_format(capi.SAMPLE_F32P).stream_pcm([planes], [60000], channels=2)
    for call in calls():
        if has_gpu:
            call()
        else:
            with pytest.raises(capi.NeedleError) as e:
                call()
            assert e.value.name == "Unknown" and "no HIP device" in str(e.value)
    if has_gpu:
        assert np.array_equal(capi.convert([x], 1, capi.SAMPLE_F32)[0], to_s16(x, capi.SAMPLE_F32))
