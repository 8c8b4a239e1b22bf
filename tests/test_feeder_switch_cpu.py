"""A lane that changes format in mid-stream (needle_hip_feeder_switch_format), without a GPU: the three new symbols through
every layer, every refusal -- each leaving lane_format, lane_segments and ready as they were --, the switch of a lane that
holds no samples (host bookkeeping only), and the host arithmetic of needle_hip_feeder_num_ready_segments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from needle_amd import capi
from tests import feeder_schedules as S
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["needle_hip_feeder_switch_format", "needle_hip_feeder_lane_segments", "needle_hip_feeder_num_ready_segments"]
INVALID, NULL = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("NullArgument")
MIX = [(2, 11025, capi.SAMPLE_S16), (3, 48000, capi.SAMPLE_F32P), (1, 22050, capi.SAMPLE_U8), (2, 44100, capi.SAMPLE_S16P)]
RATES = [11025, 44100, 22050, 48000, 96000, 32000, 12345]                           # the rates S.TILE knows, and no resampler


def test_symbols_in_every_layer(tmp_path):
    header = R.strip_comments(open(os.path.join(ROOT, "include", "needle_hip.h")).read())
    lib_rs = open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")).read()
    ffi_rs = open(os.path.join(ROOT, "rust", "needle-hip", "src", "ffi.rs")).read()
    protos = R.c_prototypes()
    fns, _, _ = R.rust_declarations()
    L = capi.lib()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(L, sym), sym
        assert sym in capi.NEEDLE_HIP_H_SYMBOLS, sym
        assert sym in fns, f"{sym} is not declared in ffi.rs"
        assert fns[sym] == protos[sym], (sym, fns[sym], protos[sym])
        assert "ffi::%s(" % sym in lib_rs, f"{sym} is not used by lib.rs"
    assert protos["needle_hip_feeder_switch_format"] == (["*mut NeedleHipFeeder", "*const usize", "*const NeedleHipLaneFormat",
                                                          "*const NeedleHipChannelMix", "usize"], "NeedleError")
    assert protos["needle_hip_feeder_lane_segments"] == (["*const NeedleHipFeeder", "usize", "*mut NeedleHipSegment", "usize", "*mut usize"],
                                                         "NeedleError")
    assert protos["needle_hip_feeder_num_ready_segments"] == (["*const NeedleHipSegment", "usize", "u32", "bool"], "usize")
    for name in ("pub fn switch_format(", "pub fn lane_segments(", "pub fn num_ready_segments("):
        assert name in lib_rs, name
    for name in ("switch_format", "lane_segments"):
        assert callable(getattr(capi.Feeder, name)), name
    assert callable(capi.num_ready_segments)
    # the struct: the header's layout, ctypes' and ffi.rs's (a NeedleHipLaneFormat, then a u64: 12 + 4 of padding + 8)
    fields = [("format", None), ("frames", None)]
    c = R.c_layout({"NeedleHipSegment": fields}, str(tmp_path))
    assert c[("NeedleHipSegment", "size")] == C.sizeof(capi.CSegment) == 24
    for f, _ in fields:
        assert c[("NeedleHipSegment", f)] == getattr(capi.CSegment, f).offset
    body = re.search(r"#\[repr\(C\)\]\s*(?:#\[[^\]]*\]\s*)*pub struct NeedleHipSegment\s*\{(.*?)\}", ffi_rs, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*:\s*(\w+)\s*,", body) == [("format", "NeedleHipLaneFormat"), ("frames", "u64")]


def state(f):
    return [(f.lane_format(k), f.lane_segments(k), f.ready(k)) for k in range(f.lanes)]


def switch(f, lanes, formats, mixes=None, null=()):
    """The C call itself, so that NULL arrays can be passed."""
    arr = None if "lanes" in null else (C.c_size_t * max(len(lanes), 1))(*lanes)
    fm = None if "formats" in null else capi._lane_formats(formats)
    mx = None if mixes is None else capi._channel_mixes(mixes)
    return capi.lib().needle_hip_feeder_switch_format(None if "feeder" in null else f._h, arr, fm, mx, len(lanes))


def test_every_refusal_leaves_the_feeder_as_it_was():
    L = capi.lib()
    f = capi.Feeder.with_formats(MIX, 2)
    gpu = capi.device_count() > 0
    pcm = np.zeros(2 * 11025 * 3, dtype=np.int16)
    if gpu:                                                                         # lane 0 holds a stream, lane 2 is finished
        f.feed([pcm, None, None, None])
        f.finish([2])
    before = state(f)
    assert before[0] == (MIX[0], [(MIX[0], len(pcm) // 2 if gpu else 0)], before[0][2])
    ok = (1, 8000, capi.SAMPLE_S16)
    stereo_mix = capi.ChannelMix.of([32768, 0], [0, 32768])
    refusals = [
        ([4], [ok], None),                                                          # lane range
        ([0, 4], [ok, ok], None),                                                   # ... in the last entry
        ([0], [(0, 11025, 1)], None), ([0], [(9, 11025, 1)], None),                 # format limits
        ([0], [(1, 1999, 1)], None), ([0], [(1, 768001, 1)], None), ([0], [(1, 11025, 10)], None), ([0], [(1, 11025, -1)], None),
        ([1, 0], [ok, (1, 44101, capi.SAMPLE_S16)], None),                          # no resampler design, in the last entry
        ([0, 1], [(6, 48000, capi.SAMPLE_S16), ok], [stereo_mix, None]),            # a mix of another channel count
        ([1, 0], [ok, (2, 48000, capi.SAMPLE_S16)], [None, capi.ChannelMix.of([32768, 32768], [0, 0])]),   # a row sum above 65535
        ([1, 0], [ok, (2, 48000, capi.SAMPLE_S16)], [None, capi.ChannelMix.of([40000, 0], [0, 0])]),       # a coefficient out of range
        ([0, 1, 0], [ok, ok, ok], None),                                            # a lane named twice
        ([3, 3], [ok, ok], None),
    ]
    if gpu:
        refusals.append(([0, 2], [ok, ok], None))                                   # a finished lane, in the last entry
    for lanes, formats, mixes in refusals:
        assert switch(f, lanes, formats, mixes) == INVALID, (lanes, formats)
        assert L.needle_hip_last_error_message()
        assert state(f) == before, (lanes, formats)
        with pytest.raises(capi.NeedleError) as e:
            f.switch_format(lanes, formats, mixes)
        assert e.value.code == INVALID and state(f) == before and f.formats == MIX
    assert switch(f, [0], [ok], null=("feeder",)) == NULL
    assert switch(f, [0], [ok], null=("lanes",)) == NULL
    assert switch(f, [0], [ok], null=("formats",)) == NULL
    assert state(f) == before
    # lane_segments' own arguments
    count, out = C.c_size_t(), (capi.CSegment * 4)()
    assert L.needle_hip_feeder_lane_segments(f._h, 4, out, 4, C.byref(count)) == INVALID
    assert L.needle_hip_feeder_lane_segments(None, 0, out, 4, C.byref(count)) == NULL
    assert L.needle_hip_feeder_lane_segments(f._h, 0, out, 4, None) == NULL
    assert L.needle_hip_feeder_lane_segments(f._h, 0, None, 4, C.byref(count)) == NULL
    assert L.needle_hip_feeder_lane_segments(f._h, 0, None, 0, C.byref(count)) == 0 and count.value == 1
    # a feeder of one format for all lanes refuses, whatever is asked
    g = capi.Feeder(3, 2, 48000, capi.SAMPLE_S16, 2)
    g_before = state(g)
    assert g_before[0][1] == [((2, 48000, capi.SAMPLE_S16), 0)]
    assert switch(g, [0], [(2, 48000, capi.SAMPLE_S16)]) == INVALID and switch(g, [1], [ok]) == INVALID
    with pytest.raises(capi.NeedleError) as e:
        g.switch_format([0], [ok])
    assert e.value.code == INVALID and state(g) == g_before and g.formats is None
    # the refused feeder still feeds by the formats it had (an empty feed needs no device)
    ptrs = (C.c_void_p * 7)(*([pcm.ctypes.data] * 7))
    assert L.needle_hip_feeder_feed(f._h, ptrs, (C.c_size_t * 4)(0, 0, 0, 0)) == 0
    assert L.needle_hip_feeder_feed(f._h, ptrs, (C.c_size_t * 4)(0, 4, 0, 0)) == INVALID     # lane 1 still has three channels


def test_a_poisoned_feeder_returns_its_error():
    """Without a device a feed of samples fails and poisons the feeder; a switch then answers with that error, for a lane
    without samples too, and changes nothing.  (With a device nothing here can poison a feeder: the halves before it.)"""
    if capi.device_count() > 0:
        pytest.skip("a GPU is present: nothing here can poison a feeder (no test faults a device on purpose)")
    f = capi.Feeder.with_formats(MIX, 2)
    f.switch_format([1], [MIX[0]])
    with pytest.raises(capi.NeedleError) as poison:
        f.feed([np.zeros(64, dtype=np.int16), None, None, None])
    assert poison.value.code not in (0, INVALID, NULL)
    formats, segments = [f.lane_format(k) for k in range(4)], [f.lane_segments(k) for k in range(4)]
    assert switch(f, [3], [(1, 8000, capi.SAMPLE_S16)]) == poison.value.code
    assert switch(f, [9], [(1, 8000, capi.SAMPLE_S16)]) == poison.value.code
    assert [f.lane_format(k) for k in range(4)] == formats and [f.lane_segments(k) for k in range(4)] == segments


def test_a_switched_lane_without_samples_still_takes_the_audit_and_a_mix():
    """set_audit and set_lane_mix ask whether a lane holds samples in ANY segment of its stream: a lane that switched
    while empty holds none (a lane that was fed and then switched does: tests/test_gpu_feeder_switch.py)."""
    f = capi.Feeder.with_formats(MIX, 2)
    f.switch_format([0, 1], [(6, 48000, capi.SAMPLE_S16), MIX[1]])
    f.set_lane_mix([0], [capi.channel_mix_default(0x60F)])
    with pytest.raises(capi.NeedleError) as e:
        f.set_lane_mix([1], [capi.channel_mix_default(0x60F)])                      # three channels there
    assert e.value.code == INVALID
    if capi.device_count() > 0:                                                     # (the audit's counts live on the device)
        f.set_audit(True)
        f.set_audit(False)
    assert f.lane_segments(0) == [(MIX[0], 0), ((6, 48000, capi.SAMPLE_S16), 0)]


def test_a_lane_without_samples_switches_without_a_device():
    f = capi.Feeder.with_formats(MIX, 2)
    new1, new3 = (6, 96000, capi.SAMPLE_F64), (1, 11025, capi.SAMPLE_S16)
    f.switch_format([1, 3], [new1, new3], [capi.channel_mix_default(0x60F), None])
    assert [f.lane_format(k) for k in range(4)] == [MIX[0], new1, MIX[2], new3] == f.formats
    assert f.lane_segments(0) == [(MIX[0], 0)] and f.lane_segments(2) == [(MIX[2], 0)]
    assert f.lane_segments(1) == [(MIX[1], 0), (new1, 0)] and f.lane_segments(3) == [(MIX[3], 0), (new3, 0)]
    assert all(f.ready(k) == (0, 0, False) for k in range(4))
    f.switch_format([1], [new1])                                                    # nothing changes: a segment all the same
    assert f.lane_segments(1) == [(MIX[1], 0), (new1, 0), (new1, 0)] and f.ready(1) == (0, 0, False)
    # at most `cap` are written, the count is the number there are
    count, out = C.c_size_t(), (capi.CSegment * 3)()
    out[2].frames = 77
    assert capi.lib().needle_hip_feeder_lane_segments(f._h, 1, out, 2, C.byref(count)) == 0 and count.value == 3
    assert (out[0].format.sample_rate, out[1].format.sample_rate, out[2].frames) == (48000, 96000, 77)
    # the pointer array is now counted by the new formats: lane 1 is interleaved, lane 3 has one plane
    pcm = np.zeros(64, dtype=np.int16)
    ptrs = (C.c_void_p * 4)(*([pcm.ctypes.data] * 4))
    L = capi.lib()
    assert L.needle_hip_feeder_feed(f._h, ptrs, (C.c_size_t * 4)(0, 0, 0, 0)) == 0
    assert L.needle_hip_feeder_feed(f._h, ptrs, (C.c_size_t * 4)(0, 4, 0, 0)) == INVALID      # lane 1 has six channels now
    # reset and reset_format clear the list
    f.reset([3])
    assert f.lane_segments(3) == [(new3, 0)] and f.lane_format(3) == new3
    f.reset_format([1], [MIX[2]])
    assert f.lane_segments(1) == [(MIX[2], 0)]
    f.reset()
    assert [f.lane_segments(k) for k in range(4)] == [[(fmt, 0)] for fmt in f.formats]


def seg(rate, frames, ch=1, fmt=capi.SAMPLE_S16):
    return ((ch, rate, fmt), frames)


def out_len(frames, rate):
    return int(capi.lib().needle_hip_resample_out_len(frames, rate))


def num_kept(samples, step):
    return int(capi.lib().needle_hip_fingerprint_num_kept(samples, step))


LENGTHS = [0, 1, 7, 100, 4095, 4096, 5461, 30000, 123457, 700001]


def test_num_ready_segments_of_one_segment_is_num_ready():
    for rate in RATES:
        for n in LENGTHS:
            for step in (1, 2, 3):
                for finished in (False, True):
                    for ch in (1, 2, 6):
                        want = capi.feeder_num_ready(n, rate, ch, step, finished)
                        assert capi.num_ready_segments([seg(rate, n, ch)], step, finished) == want, (rate, n, step, finished)
    assert capi.num_ready_segments([], 1, True) == 0 and capi.num_ready_segments([seg(48000, 10 ** 6)], 0, True) == 0
    assert capi.lib().needle_hip_feeder_num_ready_segments(None, 3, 1, True) == 0
    for bad in [(0, 48000, 1), (9, 48000, 1), (1, 1999, 1), (1, 768001, 1), (1, 48000, -1), (1, 48000, 10)]:
        assert capi.num_ready_segments([seg(48000, 10 ** 6), (bad, 10 ** 6)], 1, True) == 0
        assert capi.num_ready_segments([(bad, 10 ** 6), seg(48000, 10 ** 6)], 1, False) == 0


def test_num_ready_segments_finished_is_num_kept_of_the_summed_output_lengths():
    rng = np.random.default_rng(11)
    for _ in range(200):
        k = int(rng.integers(1, 6))
        segs = [seg(int(rng.choice(RATES)), int(rng.choice(LENGTHS + [int(rng.integers(0, 400000))]))) for _ in range(k)]
        total = sum(out_len(n, fmt[1]) for fmt, n in segs)
        for step in (1, 2, 5):
            assert capi.num_ready_segments(segs, step, True) == num_kept(total, step), segs
            # unfinished: the ended segments whole, the open one by the lane arithmetic restated in tests/feeder_schedules.py
            head = sum(out_len(n, fmt[1]) for fmt, n in segs[:-1])
            have = head + S.final_outputs(segs[-1][1], segs[-1][0][1])[1]
            frames = (0 if have < S.FRAME else (have - S.FRAME) // S.HOP + 1) & ~1
            raw = max(frames - S.LATENCY, 0)
            assert capi.num_ready_segments(segs, step, False) == -(-raw // step), segs


def test_num_ready_segments_is_monotone_in_every_segment_s_length():
    rng = np.random.default_rng(12)
    for _ in range(60):
        k = int(rng.integers(1, 5))
        rates = [int(rng.choice(RATES)) for _ in range(k)]
        lens = [int(rng.integers(0, 200000)) for _ in range(k)]
        for step in (1, 3):
            for finished in (False, True):
                base = capi.num_ready_segments([seg(r, n) for r, n in zip(rates, lens)], step, finished)
                for i in range(k):
                    last = base
                    for more in (1, 2, 7, 1365, 4096, 50000):
                        grown = list(lens)
                        grown[i] += more
                        got = capi.num_ready_segments([seg(r, n) for r, n in zip(rates, grown)], step, finished)
                        assert got >= last, (rates, lens, i, more)
                        last = got


def test_num_ready_segments_at_11025_hz_only_is_the_single_stream_s_figure():
    rng = np.random.default_rng(13)
    for _ in range(100):
        lens = [int(rng.choice(LENGTHS[:8] + [int(rng.integers(0, 100000))])) for _ in range(int(rng.integers(1, 7)))]
        for step in (1, 2, 3):
            for finished in (False, True):
                segs = [seg(11025, n, ch=1 + i % 3, fmt=i % 10) for i, n in enumerate(lens)]
                assert capi.num_ready_segments(segs, step, finished) == capi.feeder_num_ready(sum(lens), 11025, 1, step, finished), lens
