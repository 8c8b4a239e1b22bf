"""PCM in the decoder's sample format on the MI355X: the conversion kernel against the numpy statement of the spec
(tests/test_sample_formats_cpu.py), and every door that takes a format -- Analyzer.run_pcm, the library's set_pcm,
stream_pcm and set_pcm_device, the WAV reader's host loop -- against the s16 path on the numpy-converted samples and
against the oracle.  Every comparison is bit-exact."""
import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests.test_gpu_library_rates import (ENDING, at_rate, hashes_of, job, oracle_hashes, results, sorted_runs, windows)
from tests.test_sample_formats_cpu import convert_spec, to_s16

pytestmark = pytest.mark.gpu
NS = O.NS
HD = 0.3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


# ---- 1. the kernel against the spec ----------------------------------------------------------------------------------
F32_EDGES = np.concatenate([
    np.array([0.5, 1.5, 2.5, -0.5, -1.5, 32767.5, 32766.5, -32768.5], np.float32) / np.float32(32768.0),   # ties
    np.array([1.0, -1.0, np.inf, -np.inf, 1e30, -1e30, np.nan, 1e-40, -1e-40, 0.0, -0.0], np.float32)])   # (1e-40: denormal)
F64_EDGES = np.concatenate([F32_EDGES.astype(np.float64), np.array([(0.5 + 2.0 ** -30) / 32768, -(0.5 + 2.0 ** -30) / 32768,
                                                                    (1.5 - 2.0 ** -30) / 32768, 1e300, -1e300])])
S32_EDGES = np.array([-2 ** 31, 2 ** 31 - 1, 65535, -1, -65537, 65536, -65536, 0], np.int32)
U8_EDGES = np.array([0, 128, 255, 127, 129, 1], np.uint8)
S16_EDGES = np.array([-32768, 32767, 0, -1, 1], np.int16)


def samples(rng, sample_format, n):
    """n samples of the format's type: noise over the whole range (floats beyond +-1 so that some clip), the edge values
    at both ends of any stream long enough (vector path and scalar tail)."""
    base = sample_format % 5
    if base == capi.SAMPLE_U8:
        x, edges = rng.integers(0, 256, n, dtype=np.int64).astype(np.uint8), U8_EDGES
    elif base == capi.SAMPLE_S16:
        x, edges = rng.integers(-32768, 32768, n, dtype=np.int64).astype(np.int16), S16_EDGES
    elif base == capi.SAMPLE_S32:
        x, edges = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32), S32_EDGES
    elif base == capi.SAMPLE_F32:
        x, edges = (rng.random(n, dtype=np.float32) * np.float32(2.2) - np.float32(1.1)), F32_EDGES
        x[::3] = np.rint(x[::3] * np.float32(65536.0)) / np.float32(65536.0)          # many exact ties (k + 0.5) / 32768
    else:
        x, edges = rng.random(n) * 2.2 - 1.1, F64_EDGES
        x[::3] = np.rint(x[::3] * 65536.0) / 65536.0
    if n >= 2 * len(edges):
        x[: len(edges)] = edges
        x[n - len(edges):] = edges
    elif n:
        x[:] = np.resize(edges, n)
    return x


def stream_of(x, channels, sample_format):
    """What capi.convert / run_pcm take for the interleaved samples x: x itself, or its planes."""
    if not capi.sample_format_planar(sample_format):
        return x
    frames = len(x) // channels
    return [np.ascontiguousarray(x[c: frames * channels: channels]) for c in range(channels)]


def test_pinned_values_on_the_device():
    f = np.float32
    assert capi.convert([np.array([0.5, 1.5, 2.5, -0.5], f) / f(32768)], 1, capi.SAMPLE_F32)[0].tolist() == [0, 2, 2, 0]
    assert capi.convert([np.array([1.0, -1.0, 32767.5 / 32768], f)], 1, capi.SAMPLE_F32)[0].tolist() == [32767, -32768, 32767]
    assert capi.convert([np.array([np.inf, -np.inf, 1e30, np.nan, 1e-40], f)], 1, capi.SAMPLE_F32)[0].tolist() == \
        [32767, -32768, 32767, 0, 0]
    x = np.array([(0.5 + 2.0 ** -30) / 32768, 1.0, -1.0, np.nan, np.inf, 1e300])
    assert capi.convert([x], 1, capi.SAMPLE_F64)[0].tolist() == [1, 32767, -32768, 0, 32767, 32767]     # not narrowed to f32
    s32 = np.array([-2 ** 31, 2 ** 31 - 1, 65535, -1, -65537], np.int32)
    assert capi.convert([s32], 1, capi.SAMPLE_S32)[0].tolist() == [-32768, 32767, 0, -1, -2]
    assert capi.convert([np.array([0, 128, 255], np.uint8)], 1, capi.SAMPLE_U8)[0].tolist() == [-32768, 0, 32512]
    planes = [np.array([1, 2, 3], np.int16), np.array([4, 5, 6], np.int16)]
    assert capi.convert([planes], 2, capi.SAMPLE_S16P)[0].tolist() == [1, 4, 2, 5, 3, 6]
    p, n, out = (capi.C.c_void_p * 1)(s32.ctypes.data), (capi.C.c_size_t * 1)(5), np.zeros(5, np.int16)
    for bad in (-1, 10, 12):
        assert capi.lib().needle_hip_convert_host(p, n, 1, 1, bad, (capi.C.c_void_p * 1)(out.ctypes.data)) == 3


@pytest.mark.parametrize("sample_format", range(10))
def test_convert_equals_the_numpy_spec(sample_format, monkeypatch):
    """All ten formats x channels 1, 2, 6 x streams of 0, 1, 7, 8, 9 and 2.5 M + C frames with a partial trailing frame,
    edge values at both ends: once in one batch, once cut small through NEEDLE_HIP_MAX_BATCH_VALUES."""
    rng = np.random.default_rng(100 + sample_format)
    for ch in (1, 2, 6):
        raw, lens = [], []
        for frames in (0, 1, 7, 8, 9, 2_500_000 + ch):
            raw.append(samples(rng, sample_format, frames * ch + (ch - 1)))
            lens.append(len(raw[-1]))
        streams = [stream_of(x, ch, sample_format) for x in raw]
        want = [convert_spec(x, ch, sample_format % 5) for x in raw]
        got = capi.convert(streams, ch, sample_format, num_values=lens)
        for g, w, x in zip(got, want, raw):
            assert len(g) == len(x) // ch * ch and np.array_equal(g, w), (sample_format, ch, len(x))
        monkeypatch.setenv("NEEDLE_HIP_MAX_BATCH_VALUES", str(65536 * ch + 5))
        for g, w in zip(capi.convert(streams, ch, sample_format, num_values=lens), want):
            assert np.array_equal(g, w), (sample_format, ch)
        monkeypatch.delenv("NEEDLE_HIP_MAX_BATCH_VALUES")


def test_convert_of_more_than_a_gibibyte_of_f32_in_one_stream():
    n = 280_000_000                                                                  # 1.12 GB of f32, stereo
    rng = np.random.default_rng(9)
    x = rng.random(n, dtype=np.float32)
    x *= np.float32(2.2)
    x -= np.float32(1.1)
    x[: len(F32_EDGES)] = F32_EDGES
    x[n - len(F32_EDGES):] = F32_EDGES
    got = capi.convert([x], 2, capi.SAMPLE_F32)[0]
    assert len(got) == n
    for at in range(0, n, 1 << 26):
        assert np.array_equal(got[at: at + (1 << 26)], to_s16(x[at: at + (1 << 26)], capi.SAMPLE_F32)), at


# ---- 2.-3. the four shapes through every door -------------------------------------------------------------------------
# (format, channels, rate): planar float surround at 48 kHz (the fused down-mix, then the resampler), s32 stereo at
# 44.1 kHz, 8-bit mono and f64 stereo at 11025 Hz (no resampler)
SHAPES = [(capi.SAMPLE_F32P, 6, 48000), (capi.SAMPLE_S32, 2, 44100), (capi.SAMPLE_U8, 1, 11025), (capi.SAMPLE_F64, 2, 11025)]


def in_format(s16, sample_format, seed):
    """Samples of the format that carry the s16 signal plus whatever the format can hold below it (so the conversion
    has something to round or drop).  The expected s16 is to_s16() of the result, not the input."""
    rng = np.random.default_rng(seed)
    base = sample_format % 5
    n = len(s16)
    if base == capi.SAMPLE_U8:
        return ((s16.astype(np.int32) >> 8) + 128).astype(np.uint8)
    if base == capi.SAMPLE_S32:
        return ((s16.astype(np.int64) << 16) + rng.integers(0, 65536, n)).astype(np.int32)
    if base == capi.SAMPLE_F32:
        return ((s16.astype(np.float32) + rng.random(n, dtype=np.float32) - np.float32(0.5)) / np.float32(32768.0))
    if base == capi.SAMPLE_F64:
        return (s16.astype(np.float64) + rng.random(n) * 1.4 - 0.7) / 32768.0
    return s16


def oracle_frame_hashes(pcm, ch, rate, endings=True):
    """tests/test_gpu_library_rates.py's, for 11025 Hz as well (no resampler there)."""
    hd = O.duration_from_secs_f32(HD)
    (o0, on), (e0, en, seek) = windows(len(pcm), ch, rate)

    def raw(window):
        return O.fingerprint(O.resample(window, ch, rate)) if rate != 11025 else O.fingerprint(window, channels=ch)
    op = O.step_and_timestamp(raw(pcm[ch * o0: ch * (o0 + on)]), hd)
    ed = O.step_and_timestamp(raw(pcm[ch * e0: ch * (e0 + en)]), hd, seek_to_ns=seek) if endings else []
    return O.FrameHashes(op, ed, hd)


@pytest.fixture(scope="module")
def episodes():
    return synth.make_library(4, 90.0, 20.0, outro_s=15.0)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%s-%dch-%d" % (["U8", "S16", "S32", "F32", "F64"][s[0] % 5] +
                                                                              ("P" if s[0] >= 5 else ""), s[1], s[2]))
def shape(request, episodes):
    """Per shape: the streams in the format, their numpy-converted s16, the oracle's frame hashes and results."""
    fmt, ch, rate = request.param
    raw = [in_format(at_rate(e.pcm, rate, ch, k), fmt, 50 + k) for k, e in enumerate(episodes)]
    raw[1] = raw[1][: len(raw[1]) - 1] if ch > 1 else raw[1]                          # a partial trailing frame
    s16 = [convert_spec(x, ch, fmt % 5) for x in raw]
    ref = [oracle_frame_hashes(p, ch, rate) for p in s16]
    want = O.run_with_frame_hashes(O.Comparator(include_endings=True, min_opening_duration=10 * NS,
                                                min_ending_duration=10 * NS), ref)
    assert sum(w is not None and w.opening is not None for w in want) >= 2
    return dict(fmt=fmt, ch=ch, rate=rate, raw=raw, lens=[len(x) for x in raw], streams=[stream_of(x, ch, fmt) for x in raw],
                s16=s16, ref=ref, want=want)


def names(n):
    return [f"ep{k}.wav" for k in range(n)]


def analyzer(n):
    return capi.Analyzer.from_files(names(n)).with_include_endings(True).with_ending_search_percentage(ENDING)


def test_run_pcm_with_a_format(shape):
    """Hashes and ns timestamps (opening and ending) equal the oracle's on the numpy-converted s16, and run_pcm's on it."""
    n = len(shape["raw"])
    got = analyzer(n).run_pcm(shape["streams"], channels=shape["ch"], sample_rate=shape["rate"], sample_format=shape["fmt"])
    plain = analyzer(n).run_pcm(shape["s16"], channels=shape["ch"], sample_rate=shape["rate"])
    for v in range(n):
        assert hashes_of(got[v]) == oracle_hashes(shape["ref"][v]) == hashes_of(plain[v]), v
        assert len(hashes_of(got[v])[0]) > 50 and len(hashes_of(got[v])[2]) > 20


def new_library(n, rate, fmt=None):
    lib = capi.Library(n).include_endings(ENDING).set_sample_rate(rate)
    return lib if fmt is None else lib.set_sample_format(fmt)


def device_planes(shape):
    """Every plane (or interleaved stream) in a device buffer of its own, one sample past a 16-byte boundary."""
    L = capi.lib()
    width = capi.sample_format_dtype(shape["fmt"]).itemsize
    bufs, ptrs = [], []
    for s in shape["streams"]:
        for plane in (s if capi.sample_format_planar(shape["fmt"]) else [s]):
            b = capi.DeviceBuffer(plane.nbytes + 32)
            capi.check(L.needle_hip_memcpy_h2d(b.ptr + width, plane.ctypes.data, plane.nbytes))
            bufs.append(b)
            ptrs.append(b.ptr + width)
    return bufs, ptrs


@pytest.mark.parametrize("cut", [False, True], ids=["whole", "staged-in-pieces"])
def test_library_with_a_format(shape, cut, monkeypatch):
    """set_pcm, stream_pcm and set_pcm_device (device buffers one sample off a 16-byte boundary: the scalar path) in the
    format: frame_hashes and a job's results equal the s16 library's and the oracle's, the run lists are the s16 library's."""
    fmt, ch, rate, lens, n = shape["fmt"], shape["ch"], shape["rate"], shape["lens"], len(shape["raw"])
    cmp = capi.Comparator(names(n), include_endings=True, min_opening_duration=10, min_ending_duration=10)
    plain = new_library(n, rate)
    plain.set_pcm(shape["s16"], [len(p) for p in shape["s16"]], channels=ch)
    want_results, want_runs = job(plain, cmp)
    assert results(want_results) == results(shape["want"])
    plain_hashes = [hashes_of(plain.frame_hashes(v)) for v in range(n)]
    del plain
    if cut:                                                     # many staging groups, windows in pieces
        monkeypatch.setenv("NEEDLE_HIP_MAX_BATCH_VALUES", "30001")

    def check(lib):
        got, runs = job(lib, cmp)
        assert results(got) == results(shape["want"])
        assert np.array_equal(sorted_runs(runs), sorted_runs(want_runs))
        for v in range(n):
            assert hashes_of(lib.frame_hashes(v)) == oracle_hashes(shape["ref"][v]) == plain_hashes[v], v

    lib = new_library(n, rate, fmt)
    lib.set_pcm(shape["streams"], lens, channels=ch)
    assert capi.lib().needle_hip_library_set_sample_format(lib._h, capi.SAMPLE_S16) == 3     # InvalidArgument after set_pcm ...
    check(lib)                                                                              # ... and the library still works
    audit = lib.audit()
    assert audit["mismatches"] == 0 and audit["accepted_mismatches"] == 0
    del lib

    st = new_library(n, rate, fmt)
    st.stream_pcm(shape["streams"], lens, channels=ch)
    check(st)
    del st

    bufs, ptrs = device_planes(shape)
    dev = new_library(n, rate, fmt)
    dev.set_pcm_device(ptrs, lens, channels=ch)
    del bufs                                                                   # the caller's buffers are free on return
    check(dev)


def test_mixed_null_planes_are_a_null_argument(episodes):
    ch, n = 2, len(episodes)
    planes = [[e.pcm[:40000].astype(np.float32) / 32768, e.pcm[:40000].astype(np.float32) / 32768] for e in episodes]
    lens = [80000] * n
    keep, flat = capi._format_pointers(planes, ch, capi.SAMPLE_F32P)
    flat[3] = None                                                              # video 1 keeps plane 0 only
    ptrs = (capi.C.c_void_p * len(flat))(*flat)
    sizes = (capi.C.c_size_t * n)(*lens)
    L = capi.lib()
    lib = capi.Library(n).set_sample_format(capi.SAMPLE_F32P)
    assert L.needle_hip_library_set_pcm(lib._h, ptrs, sizes, ch) == 2
    assert L.needle_hip_library_stream_pcm(lib._h, ptrs, sizes, ch) == 2
    flat[2] = None                                                              # all planes of video 1 NULL: not owned, fine
    ptrs = (capi.C.c_void_p * len(flat))(*flat)
    assert L.needle_hip_library_set_pcm(lib._h, ptrs, sizes, ch) == 0
    with pytest.raises(capi.NeedleError):
        lib.analyze(1, 1)                                                       # no PCM of video 1 on this rank
    lib.analyze(0, 1)


# ---- 4. the WAV reader's host loop is the same arithmetic -------------------------------------------------------------
def write_wav_raw(path, x, channels, rate, fmt, bits):
    payload = np.ascontiguousarray(x).tobytes()
    align = channels * bits // 8
    body = (fmt.to_bytes(2, "little") + channels.to_bytes(2, "little") + rate.to_bytes(4, "little")
            + (rate * align).to_bytes(4, "little") + align.to_bytes(2, "little") + bits.to_bytes(2, "little"))
    with open(path, "wb") as f:
        f.write(b"RIFF" + (4 + 8 + len(body) + 8 + len(payload)).to_bytes(4, "little") + b"WAVE")
        f.write(b"fmt " + len(body).to_bytes(4, "little") + body + b"data" + len(payload).to_bytes(4, "little") + payload)


@pytest.mark.parametrize("sample_format,ch,rate", [(capi.SAMPLE_F32, 2, 44100), (capi.SAMPLE_U8, 1, 11025)])
def test_wav_file_and_its_raw_samples_give_the_same_hashes(tmp_path, episodes, sample_format, ch, rate):
    """needle_audio_analyzer_run converts a float32 / 8-bit WAV on the host (wav_convert); run_pcm_format converts the
    file's raw samples on the device: the same FrameHashes."""
    raw, paths = [], []
    for k, e in enumerate(episodes[:2]):
        x = in_format(at_rate(e.pcm, rate, ch, k), sample_format, 70 + k)
        if sample_format == capi.SAMPLE_F32:
            x[100:111] = np.array([np.nan, np.inf, -np.inf, 1e30, 1.0, -1.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768,
                                   -0.5 / 32768, 1e-40], np.float32)
        p = str(tmp_path / f"e{k}.wav")
        write_wav_raw(p, x, ch, rate, 3 if sample_format == capi.SAMPLE_F32 else 1, 8 * x.dtype.itemsize)
        raw.append(x)
        paths.append(p)
    def run(an):
        return an.with_include_endings(True).with_ending_search_percentage(ENDING)
    from_files = run(capi.Analyzer.from_files(paths)).run(hash_duration=HD, persist=False)
    from_pcm = run(capi.Analyzer.from_files(paths)).run_pcm(raw, channels=ch, sample_rate=rate, sample_format=sample_format)
    for a, b in zip(from_files, from_pcm):
        assert hashes_of(a) == hashes_of(b) and len(hashes_of(a)[0]) > 50
        assert a.md5() == b.md5()


# ---- 5. the default is the old path -----------------------------------------------------------------------------------
def test_s16_launches_no_conversion(episodes):
    """An explicit S16 equals no setter, and with every kernel timed "convert" is never launched by an s16 run_pcm or an
    s16 library job (it is by an f32 one)."""
    n, ch, rate = len(episodes), 2, 48000
    pcms = [at_rate(e.pcm, rate, ch, k) for k, e in enumerate(episodes)]
    lens = [len(p) for p in pcms]
    cmp = capi.Comparator(names(n), include_endings=True, min_opening_duration=10, min_ending_duration=10)
    capi.set_kernel_timing("all")
    try:
        a = analyzer(n).run_pcm(pcms, channels=ch, sample_rate=rate)
        b = analyzer(n).run_pcm(pcms, channels=ch, sample_rate=rate, sample_format=capi.SAMPLE_S16)
        assert [hashes_of(x) for x in a] == [hashes_of(x) for x in b]
        plain, explicit = new_library(n, rate), new_library(n, rate, capi.SAMPLE_S16)
        plain.set_pcm(pcms, lens, channels=ch)
        explicit.set_pcm(pcms, lens, channels=ch)
        (res_a, runs_a), (res_b, runs_b) = job(plain, cmp), job(explicit, cmp)
        assert results(res_a) == results(res_b) and np.array_equal(sorted_runs(runs_a), sorted_runs(runs_b))
        assert [hashes_of(plain.frame_hashes(v)) for v in range(n)] == [hashes_of(explicit.frame_hashes(v)) for v in range(n)]
        capi.synchronize()
        assert capi.last_kernel_ms("resample") >= 0
        assert capi.last_kernel_ms("convert") < 0
        f32 = [p.astype(np.float32) / np.float32(32768.0) for p in pcms]
        c = analyzer(n).run_pcm(f32, channels=ch, sample_rate=rate, sample_format=capi.SAMPLE_F32)
        assert [hashes_of(x) for x in c] == [hashes_of(x) for x in a]
        capi.synchronize()
        assert capi.last_kernel_ms("convert") >= 0
    finally:
        capi.set_kernel_timing(None)
