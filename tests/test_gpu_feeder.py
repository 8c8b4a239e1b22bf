"""-m gpu: the streaming fingerprinter (needle_hip_feeder_*).  Every comparison is bit for bit: a lane's items after
`finish` against the one-shot path and the oracle over the concatenation of its chunks, whatever the cutting, the
step, the rate, the channel count and the sample format; `ready` against needle_hip_feeder_num_ready after every
feed, and the items so far a prefix that is never revised."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests.test_gpu_library_rates import FAMILIES, at_rate, hashes_of, oracle_hashes, results, windows
from tests.test_gpu_library_rates import oracle_frame_hashes as oracle_frame_hashes_at_rate
from tests.test_gpu_sample_formats import SHAPES, convert_spec, in_format, stream_of

pytestmark = pytest.mark.gpu
NS = O.NS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def signal(n, seed, rate=11025):
    """Two tones, one of them wandering, over noise: every item differs from its neighbours."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(rate)
    x = (6000 * np.sin(2 * np.pi * (220 + 30 * seed) * t) + 3000 * np.sin(2 * np.pi * 1333.0 * t * (1 + 0.1 * np.sin(t))) +
         2000 * rng.standard_normal(n))
    return np.clip(x, -32768, 32767).astype(np.int16)


def chunk_of(stream, ch, fmt, first, count):
    """Frames [first, first + count) of a stream as Feeder.feed takes them (planar: a list of planes)."""
    if count == 0:
        return None
    if capi.sample_format_planar(fmt):
        return [p[first: first + count] for p in stream]
    return stream[first * ch: (first + count) * ch]


def fed(stream, frames, cuts, step, ch=1, rate=11025, fmt=capi.SAMPLE_S16, lanes=1):
    """Feeds one lane (the last of `lanes`) chunk by chunk, checking after every feed that `ready` is the host
    arithmetic's count and that the items so far extend the ones seen before; returns the finished lane's items."""
    f = capi.Feeder(lanes, ch, rate, fmt, step)
    lane, pos, seen = lanes - 1, 0, np.zeros(0, dtype=np.uint32)
    assert sum(cuts) == frames
    for c in cuts:
        f.feed([None] * lane + [chunk_of(stream, ch, fmt, pos, c)])
        pos += c
        kept, n, finished = f.ready(lane)
        assert (n, finished) == (pos, False)
        assert kept == capi.feeder_num_ready(pos, rate, ch, step, False), (pos, kept)
        items = f.items(lane)
        assert len(items) == kept and np.array_equal(items[: len(seen)], seen), pos
        seen = items
    f.finish()
    kept, n, finished = f.ready(lane)
    assert (n, finished) == (frames, True) and kept == capi.feeder_num_ready(frames, rate, ch, step, True)
    items = f.items(lane)
    assert np.array_equal(items[: len(seen)], seen)
    for other in range(lane):
        assert f.ready(other) == (0, 0, True)
    return items


def even_cuts(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


def random_cuts(n, seed, hi=200_000, empties=True):
    rng = np.random.default_rng(seed)
    cuts = []
    while n:
        c = int(min(n, rng.integers(1, hi + 1)))
        cuts += [c, 0] if empties else [c]
        n -= c
    return cuts


# ---- cuttings x steps -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def streams():
    out = {}
    for name, n, seed in [("short", 40_000, 1), ("mid", 150_000, 2), ("long", 1_200_000, 3)]:
        pcm = signal(n, seed)
        out[name] = (pcm, O.fingerprint(pcm))
    return out


CUTTINGS = [("short", lambda n: even_cuts(n, 97)), ("mid", lambda n: even_cuts(n, 1365)), ("mid", lambda n: even_cuts(n, 2730)),
            ("mid", lambda n: even_cuts(n, 4095)), ("mid", lambda n: even_cuts(n, 4096)), ("long", lambda n: random_cuts(n, 5)),
            ("long", lambda n: [n])]


@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("which", range(len(CUTTINGS)), ids=["97", "1365", "2730", "4095", "4096", "random", "single"])
def test_every_cutting_equals_the_one_shot_and_the_oracle(streams, step, which):
    name, cut = CUTTINGS[which]
    pcm, raw = streams[name]
    want = capi.fingerprint([pcm], 1, step)[0]
    assert want.tolist() == raw[::step].tolist() and len(want) > 0
    got = fed(pcm, len(pcm), cut(len(pcm)), step)
    assert got.tolist() == want.tolist()


@pytest.mark.parametrize("step", [1, 2, 3])
def test_a_chunk_beyond_the_staging_bound_is_cut_inside(streams, step, monkeypatch):
    pcm, raw = streams["long"]
    want = capi.fingerprint([pcm], 1, step)[0]
    monkeypatch.setenv("NEEDLE_HIP_MAX_BATCH_VALUES", "70001")
    f = capi.Feeder(1, 1, 11025, capi.SAMPLE_S16, step)
    got = fed(pcm, len(pcm), [500_000, len(pcm) - 500_000], step)
    f.feed([pcm[:300_000]])
    assert f.state_bytes()[1] == 2 * 70001, "the staging holds one bound's worth of a larger feed"
    monkeypatch.delenv("NEEDLE_HIP_MAX_BATCH_VALUES")
    assert got.tolist() == want.tolist() == raw[::step].tolist()


# ---- rates, channels, formats -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def episodes():
    return synth.make_library(5, 90.0, 20.0, outro_s=15.0)


def whole_stream_window(frames, rate):
    """Frames of Analyzer's opening window with the search percentage at 1.0: the whole stream, up to the rounding of
    its duration to nanoseconds."""
    dur = O.duration_from_secs_f64(frames * (1.0 / rate))
    return min(O.duration_mul_f32(dur, 1.0) * rate // NS, frames)


def run_pcm_whole(stream, ch, rate, fmt):
    an = capi.Analyzer.from_files(["ep.wav"]).with_opening_search_percentage(1.0)
    return an.run_pcm([stream], channels=ch, sample_rate=rate, sample_format=fmt)[0].opening_data()[0]


@pytest.mark.parametrize("rate,ch", FAMILIES)
def test_kernel_families_cut_randomly(episodes, rate, ch):
    pcm = at_rate(episodes[1].pcm, rate, ch, 1)
    want = run_pcm_whole(pcm, ch, rate, capi.SAMPLE_S16)
    frames = whole_stream_window(len(pcm) // ch, rate)                          # what the analyzer fingerprinted of it
    pcm = pcm[: frames * ch]
    raw = O.fingerprint(O.resample(pcm, ch, rate))
    assert want.tolist() == raw[::2].tolist() and len(want) > 300
    got = fed(pcm, frames, random_cuts(frames, rate + ch, hi=200_000), 2, ch=ch, rate=rate)
    assert got.tolist() == want.tolist()
    odd = fed(pcm, frames, random_cuts(frames, rate, hi=30_000, empties=False), 3, ch=ch, rate=rate)
    assert odd.tolist() == raw[::3].tolist()


@pytest.mark.parametrize("fmt,ch,rate", SHAPES)
def test_sample_formats_cut_randomly(episodes, fmt, ch, rate):
    x = in_format(at_rate(episodes[2].pcm, rate, ch, 2), fmt, 52)
    want = run_pcm_whole(stream_of(x, ch, fmt), ch, rate, fmt)
    frames = whole_stream_window(len(x) // ch, rate)                            # what the analyzer fingerprinted of it
    x = x[: frames * ch]
    s16 = convert_spec(x, ch, fmt % 5)
    stream = stream_of(x, ch, fmt)
    raw = O.fingerprint(O.resample(s16, ch, rate)) if rate != 11025 else O.fingerprint(s16, channels=ch)
    assert want.tolist() == raw[::2].tolist() and len(want) > 300
    got = fed(stream, frames, random_cuts(frames, 7 * fmt + ch), 2, ch=ch, rate=rate, fmt=fmt, lanes=2)
    assert got.tolist() == want.tolist()
    one = fed(stream, frames, random_cuts(frames, fmt, hi=50_000, empties=False), 1, ch=ch, rate=rate, fmt=fmt)
    assert one.tolist() == raw.tolist()


# ---- many lanes ---------------------------------------------------------------------------------------------------------
def test_lanes_of_different_lengths_in_lock_step():
    """Six lanes fed one second at a time: they run out -- and are finished -- at different feeds, one holds fewer than
    4096 samples, one is never fed, and one is reset after its first stream and fed a second one."""
    step, sec = 2, 11025
    lens = [300_000, 150_000, 3_000, 0, 220_500, 90_000]
    pcm = [signal(n, 10 + k) for k, n in enumerate(lens)]
    second = signal(130_000, 30)
    want = capi.fingerprint(pcm + [second], 1, step)
    f = capi.Feeder(6, 1, 11025, capi.SAMPLE_S16, step)
    pos, live, reused, first_of_5 = [0] * 6, set(range(6)) - {3}, False, None
    src = list(pcm)
    while live:
        chunks = [None] * 6
        for k in live:
            chunks[k] = src[k][pos[k]: pos[k] + sec]
            pos[k] += len(chunks[k])
        f.feed(chunks)
        done = [k for k in sorted(live) if pos[k] >= len(src[k])]
        if done:
            f.finish(done)
        for k in range(6):
            kept, n, finished = f.ready(k)
            assert n == min(pos[k], len(src[k])) and finished == (k != 3 and (k not in live or k in done))
            assert kept == capi.feeder_num_ready(n, 11025, 1, step, finished)
        live -= set(done)
        if 5 in done and not reused:
            first_of_5 = f.items(5)
            with pytest.raises(capi.NeedleError) as e:                         # finished: no more PCM until it is reset
                f.feed([None] * 5 + [second[:100]])
            assert e.value.name == "InvalidArgument"
            f.reset([5])
            assert f.ready(5) == (0, 0, False)
            src[5], pos[5], reused = second, 0, True
            live.add(5)
    f.finish()                                                                 # the lane that was never fed
    assert f.ready(3) == (0, 0, True) and f.ready(2)[0] == 0
    for k in range(5):
        assert f.items(k).tolist() == want[k].tolist(), k
    assert first_of_5.tolist() == want[5].tolist() and f.items(5).tolist() == want[6].tolist()
    assert sum(len(w) for w in want) > 200 and min(len(want[k]) for k in (0, 1, 4, 5, 6)) > 20


# ---- exactly once, same decisions -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contested():
    """Streams the one-shot itself recomputes items of: the adversarial corpus of the certification (parameter vectors;
    the PCM is regenerated) end to end in one stream, and two episodes of the hostile corpus."""
    spec = importlib.util.spec_from_file_location("fuzz_cert_adversarial", os.path.join(ROOT, "tools", "fuzz_cert_adversarial.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    corpus = json.load(open(os.path.join(ROOT, "tests", "golden", "cert_adversarial.json")))
    thetas = [corpus["before_pair_energy"]["theta"]] + [v["theta"] for v in corpus["after_pair_energy"]["families"].values()]
    thetas += [v["theta"] for v in corpus["round6"]["families"].values()]
    adversarial = np.concatenate([fz.synth(np.array(th)) for th in thetas])
    samples = 120 * 11025
    gen = synth.DeviceLibrary(2, samples, 30.0, hostile=True)
    hostile = [gen.episode(k).copy() for k in range(2)]
    gen.free()
    return [adversarial] + hostile


def counted(fn):
    capi.cert_stats(reset=True)
    out = fn()
    return out, capi.cert_stats(reset=True)


def test_every_frame_once_and_the_one_shot_s_decisions(contested, monkeypatch):
    """cert_stats around a fed run: as many items classified and as many recomputed in f64 as in the one-shot run -- the
    accept / recompute decisions are the one-shot's, item by item, because the first-pass rows are.  Every frame pair goes
    through the first pass once: the two-pair chunks it transformed exceed the one-shot's by at most the rounding of
    one chunk per feed.  The chunks RECOMPUTED are counted per feed: a chunk that items of two feeds reach into is
    recomputed in both (from the PCM tail, into rows of its own), so that count is at least the one-shot's.  It is
    bounded too: a feed recomputes only chunks its own listed items reach into, and the ones it shares with earlier
    feeds hold frames from its first item's first frame on that an earlier item also spans -- at most 19 frames, which
    touch at most 6 chunks of four.  So the repeats are at most 6 per feed that lists an item."""
    step, size = 2, 11025 // 2                                                  # half a second: four new frames per feed
    recomputed = []
    for k, pcm in enumerate(contested):
        want, one = counted(lambda: capi.fingerprint([pcm], 1, step)[0])
        assert want.tolist() == O.fingerprint(pcm)[::step].tolist()
        cuts = even_cuts(len(pcm), size)
        got, many = counted(lambda: fed(pcm, len(pcm), cuts, step))
        assert got.tolist() == want.tolist()
        recomputed.append(one["items_recomputed"])
        assert many["items"] == one["items"] == len(want)
        assert many["items_recomputed"] == one["items_recomputed"]
        assert one["chunks"] <= many["chunks"] <= one["chunks"] + len(cuts) + 1, (one, many)
        print("chunks recomputed", k, one["chunks_recomputed"], many["chunks_recomputed"], one["items_recomputed"], len(cuts))
        listing_feeds = min(len(cuts) + 1, one["items_recomputed"])           # the feeds and the finish; one item, one feed
        assert one["chunks_recomputed"] <= many["chunks_recomputed"] <= one["chunks_recomputed"] + 6 * listing_feeds
    # the content makes the one-shot itself recompute items: the adversarial stream and the hostile corpus both
    assert recomputed[0] > 0 and sum(recomputed[1:]) > 0, recomputed
    pcm = contested[0]
    monkeypatch.setenv("NEEDLE_HIP_STFT", "f64")
    want64 = capi.fingerprint([pcm], 1, 3)[0]
    got64 = fed(pcm, len(pcm), random_cuts(len(pcm), 9, hi=60_000), 3)
    monkeypatch.delenv("NEEDLE_HIP_STFT")
    assert got64.tolist() == want64.tolist() == O.fingerprint(pcm)[::3].tolist()


# ---- bounded state -------------------------------------------------------------------------------------------------------
def test_state_does_not_grow_with_the_stream():
    """state_bytes[0] is what the feeder's carry really moved: the most bytes one lane carried from one feed to the next
    (PCM tail, source-rate tail, rows).  A lane's state after a feed is a function of where the stream stands modulo the
    resampler's tile (2352 outputs at 48 kHz) and modulo four frames (5460 outputs); a second is 11025 outputs, so the
    state repeats every lcm(2352, 5460) / gcd(11025, lcm) = 152880 / 735 = 208 feeds and ten minutes (600 feeds) have
    seen every value: the high-water is equal after 10 and after 60 minutes unless something grows with the stream.
    The bound is include/needle_hip.h's for stereo at 48 kHz; the tail must also be worth carrying (more than the 19
    frames an item reaches back)."""
    rng = np.random.default_rng(3)
    block = rng.integers(-20000, 20000, 5 * 48000 * 2, dtype=np.int16)
    bound = 117_760

    def after(minutes, seconds_per_chunk):
        f = capi.Feeder(2, 2, 48000, capi.SAMPLE_S16, 2)
        assert f.state_bytes() == (0, 0)
        n = seconds_per_chunk * 48000 * 2
        for _ in range(minutes * 60 // seconds_per_chunk):
            f.feed([block[:n], block[:n]])
        assert f.ready(0)[1] == minutes * 60 * 48000
        return f.state_bytes()
    ten, sixty, other = after(10, 1), after(60, 1), after(10, 5)
    print("state bytes", ten, sixty, other)
    assert ten == sixty
    assert 19 * 1365 * 2 < ten[0] <= bound and 19 * 1365 * 2 < other[0] <= bound
    assert ten[1] == 2 * 48000 * 2 * 2 and other[1] == 2 * block.nbytes


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_episodes_fed_by_the_second_into_ten_lanes(episodes):
    """Five episodes at 48 kHz stereo, opening and ending windows cut as the analyzer cuts them, one lane each, a second of
    every lane per feed; FrameHashes, search results and index results equal Analyzer.run_pcm's and the oracle's."""
    rate, ch, n = 48000, 2, len(episodes)
    pcms = [at_rate(e.pcm, rate, ch, k) for k, e in enumerate(episodes)]
    ref = [oracle_frame_hashes_at_rate(p, ch, rate) for p in pcms]
    names = [f"ep{k}.wav" for k in range(n)]
    plain = (capi.Analyzer.from_files(names).with_include_endings(True).with_ending_search_percentage(0.25)
             .run_pcm(pcms, channels=ch, sample_rate=rate))
    lanes, seeks = [], []
    for p in pcms:
        (o0, on), (e0, en, seek) = windows(len(p), ch, rate)
        lanes += [p[ch * o0: ch * (o0 + on)], p[ch * e0: ch * (e0 + en)]]
        seeks.append(seek)
    f = capi.Feeder(2 * n, ch, rate, capi.SAMPLE_S16, 2)
    pos = 0
    while any(pos < len(x) for x in lanes):
        f.feed([x[pos: pos + rate * ch] if pos < len(x) else None for x in lanes])
        pos += rate * ch
    with pytest.raises(capi.NeedleError):
        f.frame_hashes(0, 1, seeks[0])                                          # not finished yet
    f.finish()
    got = [f.frame_hashes(2 * v, 2 * v + 1, seeks[v], hash_duration=0.3) for v in range(n)]
    for v in range(n):
        assert hashes_of(got[v]) == oracle_hashes(ref[v]) == hashes_of(plain[v]), v
        assert got[v].hash_duration() == plain[v].hash_duration()
    opening_only = f.frame_hashes(0)
    assert hashes_of(opening_only)[:2] == hashes_of(got[0])[:2] and hashes_of(opening_only)[2:] == ([], [])
    cmp = capi.Comparator(names, include_endings=True, min_opening_duration=10, min_ending_duration=10)
    want = O.run_with_frame_hashes(O.Comparator(include_endings=True, min_opening_duration=10 * NS, min_ending_duration=10 * NS), ref)
    assert sum(w is not None and w.opening is not None for w in want) >= 3
    assert results(cmp.run_with_frame_hashes(got)) == results(cmp.run_with_frame_hashes(plain)) == results(want)
    a, b = capi.Index(cmp), capi.Index(cmp)
    a.add(got)
    b.add(plain)
    assert results(a.results()) == results(b.results()) == results(want)


# ---- configs[1]'s scale ---------------------------------------------------------------------------------------------------
def test_config_scale_opening_windows_in_five_second_chunks():
    eps = synth.make_library(28, 24 * 60.0, 90.0)
    wins = [e.pcm[: len(e.pcm) // 2] for e in eps]
    want = capi.fingerprint(wins, 1, 2)
    f = capi.Feeder(28, 1, 11025, capi.SAMPLE_S16, 2)
    size, longest = 5 * 11025, max(len(w) for w in wins)
    for pos in range(0, longest, size):
        f.feed([w[pos: pos + size] if pos < len(w) else None for w in wins])
    f.finish()
    for v in range(28):
        assert f.items(v).tolist() == want[v].tolist(), v
    assert len(want[0]) > 2500 and f.state_bytes()[1] == 28 * size * 2


# ---- the libchromaprint layer ------------------------------------------------------------------------------------------
def test_libchromaprint_feeds_the_feeder(monkeypatch):
    from tests.test_capi_cpu import _chromaprint_lib
    L = _chromaprint_lib()
    pcm = np.tile(signal(2 * 60 * 11025, 40), 10)                                # 20 minutes
    want = capi.fingerprint([pcm], 1, 1)[0]
    monkeypatch.setenv("NEEDLE_CHROMAPRINT_FEED_BLOCK", "30000")
    capi.set_kernel_timing("all")
    try:
        ctx = L.chromaprint_new(1)
        assert L.chromaprint_start(ctx, 11025, 1) == 1
        for off in range(0, len(pcm), 4096):
            assert L.chromaprint_feed(ctx, pcm[off:].ctypes.data, min(4096, len(pcm) - off)) == 1
        assert L.chromaprint_finish(ctx) == 1
        capi.synchronize()
        assert capi.last_kernel_ms("feeder_carry") >= 0, "the stream went through the feeder"
    finally:
        capi.set_kernel_timing(None)
    fp, n = C.POINTER(C.c_uint32)(), C.c_int(0)
    assert L.chromaprint_get_raw_fingerprint(ctx, C.byref(fp), C.byref(n)) == 1
    assert np.ctypeslib.as_array(fp, shape=(n.value,)).tolist() == want.tolist() and n.value > 9000
    L.chromaprint_dealloc(fp)
    L.chromaprint_free(ctx)


# ---- the one-shot paths launch what they launched ---------------------------------------------------------------------------
def test_one_shot_paths_launch_no_feeder_kernel(episodes):
    pcms = [e.pcm for e in episodes]
    capi.set_kernel_timing("all,sum")                                           # every launch since now, by kernel
    try:
        capi.fingerprint(pcms, 1, 2)
        lib = capi.Library(len(pcms))
        lib.set_pcm(pcms, [len(p) for p in pcms])
        cmp = capi.Comparator([f"ep{k}.wav" for k in range(len(pcms))], min_opening_duration=10)
        lib.job_begin(cmp, 0)
        lib.job_end(cmp, 0)
        capi.synchronize()
        assert capi.last_kernel_ms("stft_chroma32") >= 0 and capi.last_kernel_ms("features_cert") >= 0
        assert capi.last_kernel_ms("feeder_carry") < 0, "no feeder kernel in a one-shot call or a library job"
        fed(pcms[0], len(pcms[0]), even_cuts(len(pcms[0]), 11025), 2)
        capi.synchronize()
        assert capi.last_kernel_ms("feeder_carry") >= 0
    finally:
        capi.set_kernel_timing(None)
