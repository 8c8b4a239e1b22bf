"""-m gpu: channel mixes (include/needle_hip.h "Channel mixes") on the device, every comparison bit for bit against the numpy
restatement of tests/channel_mix.py: the rematrix kernel alone; a 5.1 stream against its own stereo fold-down through the
analyzer; the library; a feeder whose lanes differ in layout; the file analyzer and the command line."""
import os
import subprocess

import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests import channel_mix as M
from tests.test_gpu_convert_mono import samples, stream
from tests.test_gpu_feeder import chunk_of
from tests.test_gpu_library_rates import hashes_of, job, results
from tests.test_sample_formats_cpu import to_s16

pytestmark = pytest.mark.gpu
CHANNELS = [1, 2, 3, 6, 8]
FRAMES = [0, 1, 7, 8, 9, 2048, 2049, 4099]
U8_FRAMES = [15, 16, 17]                                                       # a lane takes 16 frames of u8
FIVE_ONE = 0x60F
INVALID = capi.ERROR_NAMES.index("InvalidArgument")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def mix_of(rows):
    return capi.ChannelMix.of(*rows)


def random_rows(rng, channels):
    """Two rows of `channels` coefficients in [-32768, 32768], signs mixed, each with sum |coef| <= 65535."""
    rows = []
    for _ in range(2):
        r = rng.integers(-32768, 32769, channels)
        while abs(r).sum() > 65535:
            r = r // 2
        rows.append([int(v) for v in r])
    return rows


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    """Every (format, channels, frames) once, in a shuffled order; (format, channels, samples, rows or None): every fifth
    stream keeps the plain average, the others get the default mix of a layout with that many channels or random rows."""
    rng = np.random.default_rng(17)
    layouts = {1: 0x4, 2: 0x3, 3: 0x7, 6: FIVE_ONE, 8: 0x63F}
    spans = []
    for fmt in range(10):
        for ch in CHANNELS:
            for frames in FRAMES + (U8_FRAMES if fmt % 5 == capi.SAMPLE_U8 else []):
                spans.append((fmt, ch, samples(frames * ch, fmt, rng)))
    spans = [spans[i] for i in rng.permutation(len(spans))]
    out = []
    for k, (fmt, ch, x) in enumerate(spans):
        rows = None if k % 5 == 0 else M.default_rows(layouts[ch]) if k % 5 == 1 else random_rows(rng, ch)
        out.append((fmt, ch, x, rows))
    return out


def spec(fmt, ch, x, rows):
    return M.plain_mono(to_s16(x, fmt), ch) if rows is None else M.fold_mono_format(x, rows[0], rows[1], fmt)


def test_rematrix_equals_the_numpy_specification_in_one_launch(batch):
    """All ten formats x C in {1, 2, 3, 6, 8} x the frame counts at the edges of a lane and of a virtual block, plain and
    mixed streams side by side, floats with NaN and both infinities; every other stream starts one sample behind a
    16-byte boundary (the scalar path).  One launch of the new kernel, none of the ingest's."""
    formats = [(ch, 48000, fmt) for fmt, ch, _, _ in batch]
    mixes = [None if rows is None else mix_of(rows) for _, _, _, rows in batch]
    assert any(np.isnan(x).any() and np.isinf(x).any() for fmt, _, x, rows in batch if fmt % 5 >= capi.SAMPLE_F32 and rows)
    capi.set_kernel_timing("all,sum")
    try:
        got = capi.rematrix_host([stream(x, ch, fmt, k % 2) for k, (fmt, ch, x, _) in enumerate(batch)], formats, mixes)
        launches = {k: capi.kernel_launches(k) for k in ("rematrix", "ingest", "convert", "downmix")}
    finally:
        capi.set_kernel_timing(None)
    assert launches == {"rematrix": 1, "ingest": 0, "convert": 0, "downmix": 0}, launches
    for k, (fmt, ch, x, rows) in enumerate(batch):
        assert got[k].dtype == np.int16 and got[k].tobytes() == spec(fmt, ch, x, rows).tobytes(), (k, fmt, ch, len(x) // ch, rows)
    # the alignment of the sources changes nothing, and the plain streams are convert_mono's
    again = capi.rematrix_host([stream(x, ch, fmt, (k + 1) % 2) for k, (fmt, ch, x, _) in enumerate(batch)], formats, mixes)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))
    plain = [k for k, b in enumerate(batch) if b[3] is None]
    mono = capi.convert_mono([stream(batch[k][2], batch[k][1], batch[k][0], 0) for k in plain], [formats[k] for k in plain])
    assert all(m.tobytes() == got[k].tobytes() for m, k in zip(mono, plain))


def test_pinned_values_clipping_and_the_bound():
    """Full scale under the 5.1 default clips (its rows sum to 32769); a caller's matrix with negative coefficients at
    sum |coef| = 65535 keeps its accumulator inside int32; the identity is the stereo rule."""
    five_one = capi.channel_mix_default(FIVE_ONE)
    bound = capi.ChannelMix.of([32768, -32767], [-32767, 32768])
    hi, lo = np.full(6 * 19, 32767, np.int16), np.full(6 * 19, -32768, np.int16)
    ends = np.array([-32768, 32767, 32767, -32768, -32768, -32768, 32767, 32767, -1, 0, 0, -1, 1, -1] * 3, np.int16)
    f32 = np.array([np.nan, 1.0, np.inf, -np.inf, -1.0, 0.25, 1e30, -1e30, 3.0 / 32768, 2.5 / 32768], np.float32)
    u8 = np.full(6 * 19, 255, np.uint8)
    cases = [
        (hi, (6, 48000, capi.SAMPLE_S16), five_one, [32767] * 19),               # (32769 * 32767 + 16384) >> 15 = 32768: clipped
        (lo, (6, 48000, capi.SAMPLE_S16), five_one, [-32768] * 19),              # (-32769 * 32768 + 16384) >> 15 = -32769: clipped
        ([hi[c::6] for c in range(6)], (6, 48000, capi.SAMPLE_S16P), five_one, [32767] * 19),
        (u8, (6, 44100, capi.SAMPLE_U8), five_one, [(32512 * 32769 + 16384) >> 15] * 19),         # 32513: the rows sum to 32769
        (ends, (2, 48000, capi.SAMPLE_S16), bound, M.fold_mono(ends, [32768, -32767], [-32767, 32768]).tolist()),
        (ends, (2, 48000, capi.SAMPLE_S16), capi.channel_mix_default(0x3), M.plain_mono(ends, 2).tolist()),
        (f32, (2, 48000, capi.SAMPLE_F32), capi.channel_mix_default(0x3), [16383, 0, -12288, 0, 2]),
    ]
    # (-32768, 32767) under [32768, -32767]: -2147418113, the most negative accumulator two channels can reach, fits int32
    assert cases[4][3][:2] == [0, 0] and 32768 * -32768 + -32767 * 32767 == -2147418113 > -2 ** 31
    assert M.fold_mono_format(f32, [32768, 0], [0, 32768], capi.SAMPLE_F32).tolist() == cases[6][3]
    got = capi.rematrix_host([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    for k, (g, c) in enumerate(zip(got, cases)):
        assert g.tolist() == c[3], (k, g.tolist(), c[3])


# ---- 2. a 5.1 stream and its stereo fold-down ------------------------------------------------------------------------------------
def whole(pcm, channels, rate, mix=None, fmt=capi.SAMPLE_S16):
    """The kept hashes of one whole stream through Analyzer.run_pcm."""
    an = capi.Analyzer.from_files(["ep.wav"]).with_opening_search_percentage(1.0).set_channel_mix(mix)
    return an.run_pcm([pcm], channels=channels, sample_rate=rate, sample_format=fmt)[0].opening_data()[0]


def test_a_surround_stream_hashes_like_its_stereo_fold_down():
    rows = M.default_rows(FIVE_ONE)
    mix = capi.channel_mix_default(FIVE_ONE)
    # 11025 Hz, s16: against the fold-down handed over as 2-channel s16 (which the stereo path reduces by (L + R) / 2)
    six = M.six_channel_signal(11025)
    stereo = M.interleave(*M.fold_stereo(six, *rows))
    folded, want, plain = whole(six, 6, 11025, mix), whole(stereo, 2, 11025), whole(six, 6, 11025)
    raw = capi.fingerprint([M.fold_mono(six, *rows), M.plain_mono(six, 6)])
    differ = int((raw[0] != raw[1]).sum())
    print("raw items", len(raw[0]), "differ", differ, "mean bits", float(np.mean([bin(a ^ b).count("1") for a, b in zip(*raw)])))
    assert len(want) > 20 and folded.tolist() == want.tolist()
    assert len(raw[0]) == 75 and differ >= 1 and (folded != plain).any()
    # 48 kHz, planar f32: against the numpy mono handed over as 1 channel (the resampler reads stereo itself)
    six48 = M.six_channel_signal(48000)
    planes = [(six48[c::6].astype(np.float32) / np.float32(32768.0)) for c in range(6)]
    assert all(to_s16(p, capi.SAMPLE_F32).tobytes() == six48[c::6].tobytes() for c, p in enumerate(planes))
    folded = whole(planes, 6, 48000, mix, capi.SAMPLE_F32P)
    want = whole(M.fold_mono(six48, *rows), 1, 48000)
    plain = whole(planes, 6, 48000, None, capi.SAMPLE_F32P)
    assert len(want) > 20 and folded.tolist() == want.tolist() and (folded != plain).any()


# ---- 3. the library --------------------------------------------------------------------------------------------------------------
def surround_of(mono, seed, stereo_only=False):
    """A 5.1 (FL FR FC LFE SL SR) stream around a mono episode: the episode in FL and, quieter, in FR; other notes in the
    centre, a rumbling LFE, quiet surrounds -- or, stereo_only, a stereo episode in a six-channel container."""
    n, rng = len(mono), np.random.default_rng(seed)
    t = np.arange(n) / 11025.0
    x = np.zeros((n, 6), dtype=np.int64)
    x[:, 0] = mono
    x[:, 1] = mono.astype(np.int64) * 3 // 4 + rng.integers(-200, 200, n)
    if not stereo_only:
        x[:, 2] = 3000 * np.sin(2 * np.pi * (300 + 40 * seed) * t * (1 + 0.05 * np.sin(t)))
        x[:, 3] = 9000 * np.sin(2 * np.pi * 60 * t)
        x[:, 4], x[:, 5] = rng.integers(-300, 300, n), rng.integers(-300, 300, n)
    return np.clip(x, -32768, 32767).astype(np.int16).reshape(-1)


def test_library_folds_on_the_way_in():
    """Three 40 s videos sharing a 25 s intro in one six-channel library under the 5.1 default mix -- one of them a stereo
    episode in a six-channel container, two with all six channels alive: the resident hashes are run_pcm's over the numpy
    mono, through set_pcm, set_pcm_device and stream_pcm alike, and the job finds what the all-mono library finds."""
    eps = synth.make_library(3, 40.0, 25.0)
    rows, mix = M.default_rows(FIVE_ONE), capi.channel_mix_default(FIVE_ONE)
    six = [surround_of(e.pcm, k, stereo_only=k == 0) for k, e in enumerate(eps)]
    monos = [M.fold_mono(x, *rows) for x in six]
    names = [f"v{k}.wav" for k in range(3)]
    want = [hashes_of(f) for f in capi.Analyzer.from_files(names).run_pcm(monos, channels=1)]
    cmp = capi.Comparator.from_files(names).with_min_opening_duration(10)
    mono_lib = capi.Library(3)
    mono_lib.set_pcm(monos, [m.size for m in monos], channels=1)
    want_res, want_runs = job(mono_lib, cmp)
    assert all(r is not None and r.opening is not None for r in want_res)

    lib = capi.Library(3).set_channel_mix(mix)
    capi.set_kernel_timing("all,sum")
    try:
        lib.set_pcm(six, [x.size for x in six], channels=6)
        launches = {k: capi.kernel_launches(k) for k in ("rematrix", "downmix", "convert")}
    finally:
        capi.set_kernel_timing(None)
    assert launches["rematrix"] >= 1 and launches["downmix"] == launches["convert"] == 0, launches
    with pytest.raises(capi.NeedleError):
        lib.set_channel_mix(None)                                              # like set_sample_format: before set_pcm only
    res, runs = job(lib, cmp)
    assert [hashes_of(lib.frame_hashes(v)) for v in range(3)] == want
    assert results(res) == results(want_res) and len(runs) == len(want_runs)

    streamed = capi.Library(3).set_channel_mix(mix)
    streamed.stream_pcm(six, [x.size for x in six], channels=6)
    assert results(job(streamed, cmp)[0]) == results(want_res)
    assert [hashes_of(streamed.frame_hashes(v)) for v in range(3)] == want
    L = capi.lib()
    bufs = [capi.DeviceBuffer(x.nbytes + 16) for x in six]
    for b, x in zip(bufs, six):
        capi.check(L.needle_hip_memcpy_h2d(b.ptr + 2, x.ctypes.data, x.nbytes))   # 2 bytes past a 16-byte boundary
    dev = capi.Library(3).set_channel_mix(mix)
    dev.set_pcm_device([b.ptr + 2 for b in bufs], [x.size for x in six], channels=6)
    assert results(job(dev, cmp)[0]) == results(want_res)
    assert [hashes_of(dev.frame_hashes(v)) for v in range(3)] == want
    # without the mix the six-channel library is today's: the plain average, another set of hashes
    plain = capi.Library(3)
    plain.set_pcm(six, [x.size for x in six], channels=6)
    job(plain, cmp)
    today = [hashes_of(f) for f in capi.Analyzer.from_files(names).run_pcm([M.plain_mono(x, 6) for x in six], channels=1)]
    assert [hashes_of(plain.frame_hashes(v)) for v in range(3)] == today and today[1] != want[1]


# ---- 4. the feeder ---------------------------------------------------------------------------------------------------------------
FEEDER_LANES = [(2, 44100, capi.SAMPLE_S16), (6, 48000, capi.SAMPLE_S16), (8, 48000, capi.SAMPLE_F32P)]
# chunks per round, in frames: ragged, a 1-frame chunk, an empty feed for every lane at some point
ROUNDS = [(44100, 1, 30000), (0, 47999, 1), (1, 100000, 0), (88199, 0, 97999), (70000, 100000, 100000), (62300, 40000, 60000)]


def feeder_streams():
    """6 s per lane: stereo, 5.1 and 7.1 (planar f32), with the numpy mono each must land as."""
    seven = 0x63F
    rng = np.random.default_rng(23)
    stereo = M.six_channel_signal(44100, 6.0).reshape(-1, 6)[:, :2].reshape(-1).copy()
    six = M.six_channel_signal(48000, 6.0, seed=9)
    eight = np.concatenate([M.six_channel_signal(48000, 6.0, seed=11).reshape(-1, 6),
                            rng.integers(-400, 400, (48000 * 6, 2)).astype(np.int16)], axis=1)
    planes = [(eight[:, c].astype(np.float32) / np.float32(32768.0)) for c in range(8)]
    streams = [stereo, six, planes]
    monos = [M.plain_mono(stereo, 2), M.fold_mono(six, *M.default_rows(FIVE_ONE)), M.fold_mono(eight.reshape(-1), *M.default_rows(seven))]
    mixes = [None, capi.channel_mix_default(FIVE_ONE), capi.channel_mix_default(seven)]
    return streams, monos, mixes


def feed_rounds(f, streams):
    pos, staged = [0, 0, 0], 0
    for chunks in ROUNDS:
        f.feed([chunk_of(streams[i], FEEDER_LANES[i][0], FEEDER_LANES[i][2], pos[i], c) for i, c in enumerate(chunks)])
        pos = [p + c for p, c in zip(pos, chunks)]
        staged += any(chunks)
    f.feed([None, None, None])                                                 # nothing for any lane: no round
    f.finish()
    assert pos == [6 * 44100, 6 * 48000, 6 * 48000] and [sum(r[i] for r in ROUNDS) for i in range(3)] == pos
    return staged


def test_feeder_lanes_of_three_layouts_in_one_launch_per_round():
    streams, monos, mixes = feeder_streams()
    step = 2                                                                   # what a hash duration of 0.3 s keeps
    one_shot = [capi.Analyzer.from_files(["ep.wav"]).with_opening_search_percentage(1.0)
                .run_pcm([m], channels=1, sample_rate=FEEDER_LANES[i][1], hash_duration=0.3)[0].opening_data()[0] for i, m in enumerate(monos)]
    f = capi.Feeder.with_formats(FEEDER_LANES, step)
    f.set_lane_mix([1, 2], mixes[1:])
    # a refused call changes nothing, not for the lanes named before the bad one either
    with pytest.raises(capi.NeedleError) as e:
        f.set_lane_mix([1, 0], [None, mixes[1]])                               # lane 0 is stereo: a 6-channel mix does not fit
    assert e.value.code == INVALID
    capi.set_kernel_timing("all,sum")
    try:
        staged = feed_rounds(f, streams)
        launches = {k: capi.kernel_launches(k) for k in ("rematrix", "ingest", "convert", "downmix")}
    finally:
        capi.set_kernel_timing(None)
    assert launches == {"rematrix": staged, "ingest": 0, "convert": 0, "downmix": 0} and staged == len(ROUNDS), launches
    for i in range(3):
        assert f.ready(i)[1:] == (6 * FEEDER_LANES[i][1], True)
        assert len(one_shot[i]) > 10 and f.items(i).tolist() == one_shot[i].tolist(), i
    # Mono tails whatever the layout.  include/needle_hip.h: 76 176 B for a mono lane at 11025 Hz, plus the inputs of one
    # resampler tile and its filter's length per tail channel at another rate: 117 760 B for STEREO at 48 kHz, so
    # (117 760 - 76 176) / 2 = 20 792 B of it for MONO there, the larger of this feeder's two rates (a 44.1 kHz tile reads
    # half as many inputs).
    assert 0 < f.state_bytes()[0] <= 76_176 + (117_760 - 76_176) // 2, f.state_bytes()
    # a lane that holds samples keeps its mix; after reset it may take another
    with pytest.raises(capi.NeedleError) as e:
        f.set_lane_mix([1], [None])
    assert e.value.code == INVALID
    f.reset([1])
    f.set_lane_mix([1], [None])
    f.set_lane_mix([1], [mixes[1]])
    f.reset_format([1], [FEEDER_LANES[1]])                                     # clears the lane's mix: the plain average again
    f.feed([None, streams[1], None])
    f.finish([1])
    plain = capi.Analyzer.from_files(["ep.wav"]).with_opening_search_percentage(1.0).run_pcm(
        [M.plain_mono(streams[1], 6)], channels=1, sample_rate=48000)[0].opening_data()[0]
    assert f.items(1).tolist() == plain.tolist() != one_shot[1].tolist()

    # the same season without any mix launches what it always did
    g = capi.Feeder.with_formats(FEEDER_LANES, step)
    capi.set_kernel_timing("all,sum")
    try:
        staged = feed_rounds(g, streams)
        launches = {k: capi.kernel_launches(k) for k in ("rematrix", "ingest")}
    finally:
        capi.set_kernel_timing(None)
    assert launches == {"rematrix": 0, "ingest": staged}, launches
    assert g.items(0).tolist() == one_shot[0].tolist() and g.items(1).tolist() == plain.tolist()


# ---- 5. the file analyzer and the command line ---------------------------------------------------------------------------------------
def test_files_with_a_channel_mask_are_folded_by_their_layout(tmp_path):
    """A six-channel EXTENSIBLE WAV with mask 0x60F and the WAV of its stereo fold-down: with --layout-downmix (and with
    set_layout_downmix) their hashes are equal; without it the six-channel file's are today's plain-average ones.  A
    six-channel file without a mask keeps the plain average either way."""
    exe = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "bin", "needle")
    six = M.six_channel_signal(11025, 24.0)
    rows = M.default_rows(FIVE_ONE)
    paths = [str(tmp_path / n) for n in ("six.wav", "stereo.wav", "unmasked.wav")]
    M.write_wav(paths[0], six, 6, 11025, mask=FIVE_ONE)
    M.write_wav(paths[1], M.interleave(*M.fold_stereo(six, *rows)), 2, 11025)
    M.write_wav(paths[2], six, 6, 11025)
    plain = capi.Analyzer.from_files(["six.wav"]).run_pcm([M.plain_mono(six, 6)], channels=1)[0].opening_data()[0].tolist()

    def disk(p):
        rc, fh = O.frame_hashes_read(p[:-4] + ".needle.dat")
        assert rc == 0
        return [h for h, _ in fh.opening]
    r = subprocess.run([exe, "analyze", "--layout-downmix", "--force"] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    with_flag = [disk(p) for p in paths]
    assert len(with_flag[0]) > 20 and with_flag[0] == with_flag[1] and with_flag[2] == plain != with_flag[0]
    r = subprocess.run([exe, "analyze", "--force"] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert disk(paths[0]) == plain == disk(paths[2]) and disk(paths[1]) == with_flag[1]
    # the same through the handle, nothing persisted
    got = capi.Analyzer.from_files(paths, force=True).set_layout_downmix(True).run()
    assert [g.opening_data()[0].tolist() for g in got] == with_flag
    got = capi.Analyzer.from_files(paths, force=True).run()
    assert [g.opening_data()[0].tolist() for g in got] == [plain, with_flag[1], plain]
    # `needle search --analyze` takes the flag too: the six-channel file and its fold-down then match over their whole openings
    for flag, found in (["--layout-downmix"], True), ([], None):
        r = subprocess.run([exe, "search", "--analyze", "--min-opening-duration", "5"] + flag + paths[:2], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        if found:
            assert r.stdout.count("* Opening") == 2, r.stdout
