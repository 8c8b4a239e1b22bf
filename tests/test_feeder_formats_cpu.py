"""A feeder whose lanes have formats of their own, without a GPU: the four new symbols through every layer, the argument
errors of needle_hip_feeder_new_lanes (answered before a device is needed), the layout of feed's pointer array for a
mixture of interleaved and planar lanes, and needle_hip_feeder_num_ready per lane against the restated lane arithmetic
for lanes of different rates in one schedule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from needle_amd import capi
from tests import feeder_formats as F
from tests import feeder_schedules as S
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["needle_hip_feeder_new_lanes", "needle_hip_feeder_lane_format", "needle_hip_feeder_reset_format",
           "needle_hip_convert_mono_host"]
INVALID, NULL = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("NullArgument")
MIX = [(2, 11025, capi.SAMPLE_S16), (3, 48000, capi.SAMPLE_F32P), (1, 22050, capi.SAMPLE_U8), (2, 44100, capi.SAMPLE_S16P)]


def test_symbols_in_every_layer(tmp_path):
    header = R.strip_comments(open(os.path.join(ROOT, "include", "needle_hip.h")).read())
    lib_rs = open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")).read()
    protos = R.c_prototypes()
    fns, structs, _ = R.rust_declarations()
    L = capi.lib()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(L, sym), sym
        assert sym in capi.NEEDLE_HIP_H_SYMBOLS, sym
        assert sym in fns, f"{sym} is not declared in ffi.rs"
        assert fns[sym] == protos[sym], (sym, fns[sym], protos[sym])
        assert "ffi::%s(" % sym in lib_rs, f"{sym} is not used by lib.rs"
    assert "pub fn with_formats(" in lib_rs
    # the struct: the header's layout, ffi.rs's and ctypes'
    fields = structs["NeedleHipLaneFormat"]
    assert [f for f, _ in fields] == ["channels", "sample_rate", "format"]
    c = R.c_layout({"NeedleHipLaneFormat": fields}, str(tmp_path))
    offsets, size = R.rust_layout(fields)
    assert c[("NeedleHipLaneFormat", "size")] == size == C.sizeof(capi.CLaneFormat) == 12
    for f, off in offsets:
        assert c[("NeedleHipLaneFormat", f)] == off == getattr(capi.CLaneFormat, f).offset


def _new(formats, step=1, out=True, lanes=None, null_formats=False):
    h = C.c_void_p()
    arr = None if null_formats else capi._lane_formats(formats)
    code = capi.lib().needle_hip_feeder_new_lanes(arr, len(formats) if lanes is None else lanes, step, C.byref(h) if out else None)
    return code, h


def test_argument_errors_of_new_lanes():
    L = capi.lib()
    ok = [(1, 11025, capi.SAMPLE_S16), (6, 48000, capi.SAMPLE_F32P)]
    assert _new(ok, lanes=0)[0] == INVALID
    assert _new(ok, out=False)[0] == NULL and _new(ok, null_formats=True)[0] == NULL
    for bad in [(0, 11025, 1), (9, 11025, 1), (1, 1999, 1), (1, 768001, 1), (1, 11025, 10), (1, 11025, -1)]:
        assert _new(ok + [bad])[0] == INVALID, bad                                 # every lane is checked, the last too
        assert _new([bad] + ok)[0] == INVALID, bad
    assert _new(ok, step=0)[0] == INVALID
    # the messages are the uniform constructor's
    for bad, uniform in [((9, 11025, 1), (1, 9, 11025, 1, 1)), ((1, 1999, 1), (1, 1, 1999, 1, 1)), ((1, 11025, 10), (1, 1, 11025, 10, 1))]:
        assert _new(ok + [bad])[0] == INVALID
        mixed_message = L.needle_hip_last_error_message()
        assert L.needle_hip_feeder_new(*uniform, C.byref(C.c_void_p())) == INVALID
        assert L.needle_hip_last_error_message() == mixed_message and mixed_message
    for formats in [ok, [(8, 768000, capi.SAMPLE_F64P), (1, 2000, capi.SAMPLE_U8), (2, 11025, capi.SAMPLE_S16)]]:
        code, h = _new(formats, 2)
        assert code == 0 and h.value
        L.needle_hip_feeder_free(h)


def test_lane_format_on_both_kinds_and_reset_format_only_on_one():
    f = capi.Feeder.with_formats(MIX, 2)
    assert [f.lane_format(k) for k in range(4)] == MIX and f.lanes == 4 and f.step == 2
    g = capi.Feeder(3, 6, 48000, capi.SAMPLE_F32P, 2)
    assert [g.lane_format(k) for k in range(3)] == [(6, 48000, capi.SAMPLE_F32P)] * 3
    L = capi.lib()
    out = capi.CLaneFormat()
    assert L.needle_hip_feeder_lane_format(f._h, 4, C.byref(out)) == INVALID
    assert L.needle_hip_feeder_lane_format(f._h, 0, None) == NULL and L.needle_hip_feeder_lane_format(None, 0, C.byref(out)) == NULL
    # reset_format: a lane of a fresh feeder takes another format; bad lanes and formats change nothing
    f.reset_format([1, 3], [(1, 11025, capi.SAMPLE_F64), (8, 96000, capi.SAMPLE_S32P)])
    now = [MIX[0], (1, 11025, capi.SAMPLE_F64), MIX[2], (8, 96000, capi.SAMPLE_S32P)]
    assert [f.lane_format(k) for k in range(4)] == now
    lanes = (C.c_size_t * 2)(0, 4)
    assert L.needle_hip_feeder_reset_format(f._h, lanes, capi._lane_formats([(1, 8000, 1), (1, 8000, 1)]), 2) == INVALID
    lanes = (C.c_size_t * 2)(0, 1)
    assert L.needle_hip_feeder_reset_format(f._h, lanes, capi._lane_formats([(1, 8000, 1), (9, 8000, 1)]), 2) == INVALID
    assert L.needle_hip_feeder_reset_format(f._h, None, capi._lane_formats([(1, 8000, 1)]), 1) == NULL
    assert L.needle_hip_feeder_reset_format(f._h, lanes, None, 2) == NULL
    assert [f.lane_format(k) for k in range(4)] == now
    # the uniform constructor's feeder refuses it
    with pytest.raises(capi.NeedleError) as e:
        g.reset_format([0], [(2, 44100, capi.SAMPLE_S16)])
    assert e.value.code == INVALID
    assert [g.lane_format(k) for k in range(3)] == [(6, 48000, capi.SAMPLE_F32P)] * 3


def test_a_rate_without_a_resampler_design_is_refused_whole():
    """44101 Hz lies inside the limits, but the resampler has no design for 11025 / 44101 (its ratio is too large):
    needle_hip_feeder_new_lanes refuses it, and reset_format refuses it before any lane is reset or changed -- also the
    lanes named before it in the same call -- and the feeder goes on as it was."""
    L = capi.lib()
    assert _new([(1, 44101, capi.SAMPLE_S16)])[0] == INVALID
    assert _new([(2, 48000, capi.SAMPLE_F32), (1, 44101, capi.SAMPLE_S16)])[0] == INVALID
    assert L.needle_hip_feeder_new(1, 1, 44101, capi.SAMPLE_S16, 1, C.byref(C.c_void_p())) == INVALID
    f = capi.Feeder.with_formats(MIX, 2)
    gpu = capi.device_count() > 0
    pcm = np.zeros(2 * 11025 * 3, dtype=np.int16)
    if gpu:                                                                         # lane 0 holds a stream when it is refused
        f.feed([pcm, None, None, None])
    before = [(f.lane_format(k), f.ready(k), f.items(k).tolist()) for k in range(4)]
    assert before[0][1][1] == (len(pcm) // 2 if gpu else 0)
    for lanes, formats in [([0], [(1, 44101, capi.SAMPLE_S16)]),
                           ([2, 0, 1], [(2, 96000, capi.SAMPLE_F64), (6, 32000, capi.SAMPLE_U8P), (1, 44101, capi.SAMPLE_S32)])]:
        with pytest.raises(capi.NeedleError) as e:
            f.reset_format(lanes, formats)
        assert e.value.name == "InvalidArgument" and "rate ratio" in str(e.value)
        assert [(f.lane_format(k), f.ready(k), f.items(k).tolist()) for k in range(4)] == before
        assert f.formats == MIX
    # it still feeds: the pointer array is counted by the formats it had (an empty feed needs no device)
    ptrs = (C.c_void_p * 7)(*([pcm.ctypes.data] * 7))
    assert L.needle_hip_feeder_feed(f._h, ptrs, (C.c_size_t * 4)(0, 0, 0, 0)) == 0
    assert L.needle_hip_feeder_feed(f._h, ptrs, (C.c_size_t * 4)(0, 4, 0, 0)) == INVALID     # lane 1 still has three channels
    if gpu:
        f.feed([pcm, None, None, None])
        f.finish()
        assert f.ready(0) == (capi.feeder_num_ready(len(pcm), 11025, 2, 2, True), len(pcm), True)
    # and a reset_format that is accepted afterwards works as ever
    f.reset_format([3], [(1, 32000, capi.SAMPLE_F32)])
    assert f.lane_format(3) == (1, 32000, capi.SAMPLE_F32) and f.ready(3) == (0, 0, False)


def test_pointer_array_is_the_concatenation_of_every_lane_s_planes(monkeypatch):
    """1 pointer for an interleaved lane, channels_i for a planar one: through a recording stub in place of the
    library's feed, and through the library's own argument errors."""
    f = capi.Feeder.with_formats(MIX, 2)
    stereo = np.arange(8, dtype=np.int16)
    planes3 = [np.arange(5, dtype=np.float32) + c for c in range(3)]
    u8 = np.arange(7, dtype=np.uint8)
    planes2 = [np.arange(4, dtype=np.int16), np.arange(4, dtype=np.int16) + 9]
    real, calls = capi.lib(), []

    class Recorder:
        def needle_hip_feeder_feed(self, handle, ptrs, lens):
            calls.append(([p for p in ptrs], [n for n in lens]))
            return 0

        def __getattr__(self, name):                                                # everything else is the library's
            return getattr(real, name)
    with monkeypatch.context() as m:
        m.setattr(capi, "lib", lambda: Recorder())
        f.feed([stereo, planes3, u8, planes2])
        f.feed([None, planes3, None, None])
        f.feed([stereo, None, u8, None])
    assert capi.lib() is real
    at = lambda a: a.ctypes.data  # noqa: E731
    assert calls[0] == ([at(stereo)] + [at(p) for p in planes3] + [at(u8)] + [at(p) for p in planes2], [8, 15, 7, 8])
    assert calls[1] == ([None] + [at(p) for p in planes3] + [None] + [None, None], [0, 15, 0, 0])
    assert calls[2] == ([at(stereo), None, None, None, at(u8), None, None], [8, 0, 7, 0])
    with pytest.raises(ValueError):
        f.feed([stereo, planes3[:2], u8, planes2])                                  # a planar lane is given all its planes
    # the library counts the same way: a NULL is an error only where a lane with values has a plane
    L = capi.lib()
    seven = [at(stereo)] + [at(p) for p in planes3] + [at(u8)] + [at(p) for p in planes2]
    for hole, lens, want in [(3, (0, 15, 0, 0), NULL), (3, (0, 0, 0, 0), 0), (6, (0, 0, 0, 8), NULL), (5, (0, 0, 0, 8), NULL),
                             (4, (0, 0, 0, 0), 0), (0, (0, 0, 0, 0), 0)]:
        ptrs = list(seven)
        ptrs[hole] = None
        assert L.needle_hip_feeder_feed(f._h, (C.c_void_p * 7)(*ptrs), (C.c_size_t * 4)(*lens)) == want, (hole, lens)
    # whole frames of the lane's OWN channel count, checked for every lane before any device work
    for lens in [(7, 0, 0, 0), (0, 16, 0, 0), (0, 0, 0, 7), (8, 15, 7, 9)]:
        assert L.needle_hip_feeder_feed(f._h, (C.c_void_p * 7)(*seven), (C.c_size_t * 4)(*lens)) == INVALID, lens
    assert [f.ready(k) for k in range(4)] == [(0, 0, False)] * 4
    # convert_mono_host: the same layout, checked before any device is asked for
    out = [np.zeros(8, np.int16) for _ in range(4)]
    optrs = (C.c_void_p * 4)(*[at(o) for o in out])
    fm = capi._lane_formats(MIX)
    ptrs = list(seven)
    ptrs[2] = None
    assert L.needle_hip_convert_mono_host((C.c_void_p * 7)(*ptrs), (C.c_size_t * 4)(8, 15, 7, 8), fm, 4, optrs) == NULL
    assert L.needle_hip_convert_mono_host((C.c_void_p * 7)(*ptrs), (C.c_size_t * 4)(0, 2, 0, 0), fm, 4, optrs) == 0    # no whole frame
    assert L.needle_hip_convert_mono_host((C.c_void_p * 7)(*seven), (C.c_size_t * 4)(8, 15, 7, 8), capi._lane_formats(MIX[:3] + [(0, 1, 1)]), 4, optrs) == INVALID
    assert L.needle_hip_convert_mono_host(None, (C.c_size_t * 4)(), fm, 4, optrs) == NULL


def test_num_ready_per_lane_for_lanes_of_different_rates_in_one_schedule():
    frames = F.lane_frames()
    schedule = F.mixed_schedule(frames)
    print(F.check_mixed_conditions(schedule, frames), "rounds", len(schedule[0]))
    assert F.mixed_schedule(frames) == schedule
    assert len({rate for _, rate, _ in F.LANES}) == 4
    fed = [0] * len(frames)
    for chunks in schedule[0]:
        fed = [a + c for a, c in zip(fed, chunks)]
        for n, (ch, rate, _) in zip(fed, F.LANES):
            m = S.mirror(n, rate, ch, F.STEP)
            assert m.kept == capi.feeder_num_ready(n, rate, ch, F.STEP, False), (n, rate, ch)
    L = capi.lib()
    for n, (ch, rate, _) in zip(fed, F.LANES):
        want = int(L.needle_hip_fingerprint_num_kept(int(L.needle_hip_resample_out_len(n, rate)), F.STEP))
        assert capi.feeder_num_ready(n, rate, ch, F.STEP, True) == want > 50


def test_feed_without_a_device_fails_loudly():
    f = capi.Feeder.with_formats([(2, 48000, capi.SAMPLE_F32), (1, 11025, capi.SAMPLE_S16)], 2)
    if capi.device_count() > 0:                                       # (with one, the same calls simply work)
        f.feed([np.zeros(96000, dtype=np.float32), None])
        f.finish()
        assert f.ready(0) == (capi.feeder_num_ready(48000, 48000, 2, 2, True), 48000, True)
        return
    with pytest.raises(capi.NeedleError) as e:
        f.feed([np.zeros(96000, dtype=np.float32), None])
    assert "no HIP device" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:
        capi.convert_mono([np.zeros(16, dtype=np.float32)], [(2, 48000, capi.SAMPLE_F32)])
    assert "no HIP device" in str(e.value)
