"""-m gpu: feeder_ingest_kernel alone, through needle_hip_convert_mono_host.  One call holds every sample format x
channels {1, 2, 3, 5, 6, 8} x the frame counts at the edges of a lane (8 and 16 frames) and of a virtual block (2048 and
4096 frames), sources aligned and not; the result is compared byte for byte with (a) needle_hip_convert_host followed by
needle_hip_downmix_host and (b) a numpy restatement of the two rules of include/needle_hip.h."""
import numpy as np
import pytest

from needle_amd import capi
from tests.test_sample_formats_cpu import to_s16

pytestmark = pytest.mark.gpu
CHANNELS = [1, 2, 3, 5, 6, 8]
FRAMES = [0, 1, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 4095, 4096, 4099]
TIES = [(k + 0.5) / 32768 for k in (-3, -2, -1, 0, 1, 2, 32766, 32767, -32769)]
F64_ONLY = (0.5 + 2.0 ** -30) / 32768                                            # 1 in f64, 0 if narrowed to f32 first


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def mono_spec(x, channels, sample_format):
    """Interleaved samples -> mono s16: to_s16 per sample, then (sum of the frame) / channels truncated toward zero."""
    s = to_s16(x, sample_format).astype(np.int64).reshape(-1, channels).sum(axis=1)
    return (np.sign(s) * (np.abs(s) // channels)).astype(np.int16)


def placed(a, skew):
    """A copy of `a` whose first byte lies `skew` samples behind a 16-byte boundary."""
    raw = np.zeros(a.nbytes + 32 + a.itemsize, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16 + skew * a.itemsize
    out = raw[start: start + a.nbytes].view(a.dtype)
    out[:] = a
    assert a.size == 0 or out.ctypes.data % 16 == (skew * a.itemsize) % 16
    return out


def samples(n, sample_format, rng):
    """n interleaved samples of the format: random over its whole range (floats beyond +-1 too), the values the two
    rules turn on at both ends."""
    base = sample_format % 5
    if base == capi.SAMPLE_U8:
        x, special = rng.integers(0, 256, n).astype(np.uint8), [0, 255, 128, 127, 0, 0, 129]
    elif base == capi.SAMPLE_S16:
        x, special = rng.integers(-32768, 32768, n).astype(np.int16), [-1, 0, 32767, -32768, -1, -1, 1, -3]
    elif base == capi.SAMPLE_S32:
        x, special = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32), [-65536, 0, 2 ** 31 - 1, -2 ** 31, 65535, -1, -65537]
    else:
        dtype = capi.sample_format_dtype(sample_format)
        x = (rng.random(n) * 2.4 - 1.2).astype(dtype)
        special = [-1.0 / 32768, 0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, F64_ONLY, 1e30, -1e-40] + TIES
        special = np.array(special, dtype=dtype)
    k = min(len(special), n)
    x[:k] = special[:k]
    if n >= 2 * len(special):
        x[n - len(special):] = special
    return x


def stream(x, channels, sample_format, skew):
    """The interleaved samples as convert_mono takes them.  skew 1: the (interleaved) source or plane 1 of a planar one
    starts one sample behind a 16-byte boundary, the other planes on one."""
    if not capi.sample_format_planar(sample_format):
        return placed(x, skew)
    return [placed(np.ascontiguousarray(x[c::channels]), skew if c == min(1, channels - 1) else 0) for c in range(channels)]


@pytest.fixture(scope="module")
def mixture():
    """Every (format, channels, frames) once, in an order that puts different formats next to each other (the test
    misaligns every other span)."""
    rng = np.random.default_rng(7)
    spans = []
    for fmt in range(10):
        for ch in CHANNELS:
            for frames in FRAMES:
                spans.append((fmt, ch, samples(frames * ch, fmt, rng)))
    order = rng.permutation(len(spans))
    spans = [spans[i] for i in order]
    empty = [k for k, s in enumerate(spans) if len(s[2]) == 0 and 0 < k < len(spans) - 1]
    assert any(len(spans[k - 1][2]) and len(spans[k + 1][2]) for k in empty), "an empty span between two full ones"
    return spans


def test_pinned_values():
    """s16 extremes in all eight channels; negative sums that C's division truncates toward zero; the floating-point
    specials, alone (C = 1) and mixed."""
    hi, lo = [32767] * 8 * 17, [-32768] * 8 * 17
    f32, f64 = np.float32, np.float64
    specials = [np.nan, np.inf, -np.inf, 1.0, -1.0, 32767.5 / 32768, 1e30, 1e-40]
    cases = [
        (np.array(hi, np.int16), (8, 1, capi.SAMPLE_S16), [32767] * 17),
        (np.array(lo, np.int16), (8, 1, capi.SAMPLE_S16), [-32768] * 17),
        (np.array([-1, 0, -1, -2, 1, -2, -32768, 32767, -3, 0], np.int16), (2, 1, capi.SAMPLE_S16), [0, -1, 0, 0, -1]),
        (np.array([-1, 0, -1, -2, 0, 0, -3, -3, -2, 3, 3, 1], np.int16), (3, 1, capi.SAMPLE_S16), [0, 0, -2, 2]),
        ([np.array([-1, -7], np.int16), np.array([0, 0], np.int16)], (2, 1, capi.SAMPLE_S16P), [0, -3]),
        (np.array([-65536, 0, -65537, 65535], np.int32), (2, 1, capi.SAMPLE_S32), [0, -1]),         # (-1 + 0) / 2, (-2 + 0) / 2
        (np.array([127, 128, 128], np.uint8), (3, 1, capi.SAMPLE_U8), [-85]),                         # -256 / 3
        (np.array(specials, f32), (1, 1, capi.SAMPLE_F32), [0, 32767, -32768, 32767, -32768, 32767, 32767, 0]),
        (np.array(specials + [F64_ONLY], f64), (1, 1, capi.SAMPLE_F64), [0, 32767, -32768, 32767, -32768, 32767, 32767, 0, 1]),
        (np.array([F64_ONLY], f32), (1, 1, capi.SAMPLE_F32), [0]),
        (np.array(TIES[:6], f32), (1, 1, capi.SAMPLE_F32), [-2, -2, 0, 0, 2, 2]),                     # ties to even
        (np.array(TIES[:6], f64), (2, 1, capi.SAMPLE_F64), [-2, 0, 2]),
        (np.array([np.nan, -1.0 / 32768, np.inf, -np.inf, 1.0, 1.0], f32), (2, 1, capi.SAMPLE_F32), [0, 0, 32767]),
    ]
    got = capi.convert_mono([c[0] for c in cases], [c[1] for c in cases])
    for k, (g, c) in enumerate(zip(got, cases)):
        assert g.tolist() == c[2], (k, g.tolist(), c[2])


def test_every_format_and_channel_count_mixed_in_one_launch(mixture):
    formats = [(ch, 11025 + k, fmt) for k, (fmt, ch, _) in enumerate(mixture)]                       # (the rate is not looked at)
    streams = [stream(x, ch, fmt, k % 2) for k, (fmt, ch, x) in enumerate(mixture)]
    capi.set_kernel_timing("all,sum")
    try:
        got = capi.convert_mono(streams, formats)
        launches = {k: capi.kernel_launches(k) for k in ("ingest", "convert", "downmix")}
    finally:
        capi.set_kernel_timing(None)
    assert launches == {"ingest": 1, "convert": 0, "downmix": 0}, launches
    # (b) the numpy restatement
    for k, (fmt, ch, x) in enumerate(mixture):
        assert got[k].dtype == np.int16 and got[k].tobytes() == mono_spec(x, ch, fmt).tobytes(), (k, fmt, ch, len(x) // ch)
    # (a) convert_host, then downmix_host: per (format, channels), the spans of that kind
    for fmt in range(10):
        for ch in CHANNELS:
            mine = [k for k, s in enumerate(mixture) if s[:2] == (fmt, ch)]
            assert sorted(len(mixture[k][2]) // ch for k in mine) == FRAMES
            s16 = capi.convert([stream(mixture[k][2], ch, fmt, 0) for k in mine], ch, fmt)
            mono = capi.downmix(s16, ch)
            for k, m in zip(mine, mono):
                assert got[k].tobytes() == m.tobytes(), (k, fmt, ch)
    # the alignment of the sources changes nothing
    again = capi.convert_mono([stream(x, ch, fmt, (k + 1) % 2) for k, (fmt, ch, x) in enumerate(mixture)], formats)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))


def test_a_partial_trailing_frame_is_dropped_and_batches_are_bounded(mixture, monkeypatch):
    """num_values that are not whole frames; and the same spans cut small through NEEDLE_HIP_MAX_BATCH_VALUES: pieces of
    whole 16-frame groups, each batch one launch."""
    rng = np.random.default_rng(11)
    picks = [(fmt, ch, samples(frames * ch + ch // 2, fmt, rng)) for fmt, ch, frames in
             [(capi.SAMPLE_F32, 5, 4099), (capi.SAMPLE_U8, 3, 4097), (capi.SAMPLE_S16, 2, 0), (capi.SAMPLE_F64, 8, 2049), (capi.SAMPLE_S32, 6, 17)]]
    planar = [(capi.SAMPLE_S16P, 3, samples(3 * 2051, capi.SAMPLE_S16, rng)), (capi.SAMPLE_U8P, 2, samples(2 * 4100, capi.SAMPLE_U8, rng))]
    formats = [(ch, 48000, fmt) for fmt, ch, _ in picks + planar]
    streams = [x for _, _, x in picks] + [stream(x, ch, fmt, 1) for fmt, ch, x in planar]
    num_values = [len(x) for _, _, x in picks] + [len(x) + 1 for _, _, x in planar]
    want = [mono_spec(x[: len(x) // ch * ch], ch, fmt) for fmt, ch, x in picks + planar]
    got = capi.convert_mono(streams, formats, num_values)
    assert [g.tobytes() for g in got] == [w.tobytes() for w in want]
    monkeypatch.setenv("NEEDLE_HIP_MAX_BATCH_VALUES", "6000")
    capi.set_kernel_timing("ingest,sum")
    try:
        cut = capi.convert_mono(streams, formats, num_values)
        launches = capi.kernel_launches("ingest")
    finally:
        capi.set_kernel_timing(None)
        monkeypatch.delenv("NEEDLE_HIP_MAX_BATCH_VALUES")
    assert [g.tobytes() for g in cut] == [w.tobytes() for w in want]
    assert launches >= sum(num_values) // 6000, launches
