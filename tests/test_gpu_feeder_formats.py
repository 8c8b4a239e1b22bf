"""-m gpu: a feeder whose lanes have a rate, a channel count and a sample format of their own (Feeder.with_formats).
Six lanes of six formats fed out of step in one feeder, every comparison bit for bit: the one-shot path, the oracle, a
uniform feeder over the same stream, the host arithmetic of `ready`; the launches of a round; the mono state; a lane
that changes its format with its next stream; the audit; and a season of four formats down the chain into the search."""
import os
import subprocess
import sys

import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests import feeder_formats as F
from tests import feeder_schedules as S
from tests.test_gpu_crossmatcher import by_pair
from tests.test_gpu_crossmatcher_regions import one_shot as regions_one_shot
from tests.test_gpu_feeder import chunk_of, signal
from tests.test_gpu_feeder_ragged import HASH_DURATION, content, one_shot
from tests.test_gpu_library_rates import at_rate, hashes_of, oracle_hashes, results, windows
from tests.test_gpu_sample_formats import convert_spec, in_format, oracle_frame_hashes, stream_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = O.NS
STEP = F.STEP
PARENT_KERNELS = {"feeder_carry", "stft_chroma32", "features_cert", "stft_fallback", "fixup_items"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


# ---- the six lanes ------------------------------------------------------------------------------------------------------------
_LANES = {}


def lanes():
    """The six lanes, made once: their streams (cut to what the analyzer fingerprints of them), frames, the one-shot
    path's items and the oracle's."""
    if not _LANES:
        streams, frames, want, raw = [], [], [], []
        for k in range(len(F.LANES)):
            cfg = F.lane_config(k)
            c = content(cfg)
            streams.append(c["streams"][0])
            frames.append(c["frames"][0])
            want.append(one_shot(cfg, c)[0])
            raw.append(c["raw"][0][::STEP])
        assert frames == F.lane_frames()
        _LANES.update(streams=streams, frames=frames, want=want, raw=raw)
    return _LANES


def feed_mixed(f, formats, streams, schedule, after_round=None):
    """tests/test_gpu_feeder_ragged.py's driver with a format per lane: one feed per round with every lane's chunk in the
    same call, then `finish` for the lanes the schedule ends there; after every round `ready` is the host arithmetic's
    count at the lane's own rate and the items so far are the ones seen before plus a suffix."""
    rounds, finishes = schedule
    n = len(streams)
    streams, formats = list(streams), list(formats)
    pos, finished = [0] * n, [False] * n
    seen = [np.zeros(0, dtype=np.uint32) for _ in range(n)]
    for r, (chunks, done) in enumerate(zip(rounds, finishes)):
        f.feed([chunk_of(streams[i], formats[i][0], formats[i][2], pos[i], c) for i, c in enumerate(chunks)])
        pos = [p + c for p, c in zip(pos, chunks)]
        if done:
            f.finish(done)
            for i in done:
                finished[i] = True
        for i in range(n):
            ch, rate, _ = formats[i]
            want = (capi.feeder_num_ready(pos[i], rate, ch, f.step, finished[i]), pos[i], finished[i])
            assert f.ready(i) == want, (r, i, f.ready(i), want)
            items = f.items(i)
            assert len(items) == want[0] and np.array_equal(items[: len(seen[i])], seen[i]), (r, i)
            seen[i] = items
        if after_round:
            after_round(r, dict(streams=streams, formats=formats, pos=pos, finished=finished, seen=seen))
    assert all(finished)
    return seen


def uniform_items(stream, fmt, frames, chunk=None):
    """The stream through a feeder of needle_hip_feeder_new, in chunks of `chunk` frames (None: one feed)."""
    ch, rate, sample_format = fmt
    g = capi.Feeder(1, ch, rate, sample_format, STEP)
    pos = 0
    while pos < frames:
        c = min(chunk or frames, frames - pos)
        g.feed([chunk_of(stream, ch, sample_format, pos, c)])
        pos += c
    g.finish()
    return g.items(0)


def check_mixed_lanes():
    """Test 1's body (also run in a child process under NEEDLE_HIP_STFT=f64)."""
    d = lanes()
    schedule = F.mixed_schedule(d["frames"])
    F.check_mixed_conditions(schedule, d["frames"])
    f = capi.Feeder.with_formats(F.LANES, STEP)
    assert [f.lane_format(k) for k in range(f.lanes)] == F.LANES

    def prefix(r, st):
        for i in range(f.lanes):
            assert st["seen"][i].tolist() == d["want"][i][: len(st["seen"][i])].tolist(), (r, i)
    items = feed_mixed(f, F.LANES, d["streams"], schedule, after_round=prefix)
    for k in range(f.lanes):
        assert len(items[k]) > 50
        assert items[k].tolist() == d["want"][k].tolist(), ("one-shot", k, F.LANES[k])
        assert items[k].tolist() == d["raw"][k].tolist(), ("oracle", k, F.LANES[k])
        assert items[k].tolist() == uniform_items(d["streams"][k], F.LANES[k], d["frames"][k]).tolist(), ("uniform feeder", k)
    return f.state_bytes(), len(schedule[0])


def test_six_lanes_of_six_formats_out_of_step_equal_the_one_shot_path():
    state, rounds = check_mixed_lanes()
    print("state bytes", state, "rounds", rounds)


def test_the_same_under_the_f64_transform_in_a_child_process():
    env = dict(os.environ, NEEDLE_HIP_STFT="f64")
    code = "from tests.test_gpu_feeder_formats import check_mixed_lanes; print('mixed lanes', check_mixed_lanes(), 'ok')"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-4000:]


# ---- 2. the same format in every lane ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,seconds", [((2, 48000, capi.SAMPLE_S16), (20, 21.5, 23)), ((1, 11025, capi.SAMPLE_S16), (24, 20, 22.2))])
def test_lanes_all_given_one_format_equal_the_uniform_constructor(fmt, seconds):
    ch, rate, sample_format = fmt
    c = content(S.Config(rate, ch, sample_format, STEP, seconds, 0))
    n = len(seconds)
    a, b = capi.Feeder.with_formats([fmt] * n, STEP), capi.Feeder(n, ch, rate, sample_format, STEP)
    schedule = S.ragged_schedule(c["frames"], rate, 5)
    items = feed_mixed(a, [fmt] * n, c["streams"], schedule)
    same = feed_mixed(b, [fmt] * n, c["streams"], schedule)
    for k in range(n):
        assert len(items[k]) > 50 and items[k].tolist() == same[k].tolist() == c["raw"][k][::STEP].tolist(), k
    sa, sb = a.state_bytes(), b.state_bytes()
    print("state bytes (with_formats, uniform)", fmt, sa, sb)
    assert sa == sb if ch == 1 else sa[0] < sb[0]                                  # mono tails against stereo ones


# ---- 3. launches ----------------------------------------------------------------------------------------------------------------
def timed(fn):
    """{timer name: launches} of what fn() launches, with the events of set_kernel_timing("all,sum")."""
    from tests.test_gpu_feeder_audit import _timer_names
    names = _timer_names()
    capi.set_kernel_timing("all,sum")
    try:
        fn()
        capi.synchronize()
        shown = {k for k in names if capi.last_kernel_ms(k) >= 0}
        counts = {k: capi.kernel_launches(k) for k in names if capi.kernel_launches(k)}
        assert shown == set(counts), (shown, counts)
        return counts
    finally:
        capi.set_kernel_timing(None)


def feed_seconds(f, formats, streams, seconds, only=None):
    """`seconds` rounds of one second per lane (only: the lanes that are fed), then ready() of every lane."""
    for sec in range(seconds):
        f.feed([chunk_of(streams[i], ch, fmt, sec * rate, rate) if only is None or i in only else None
                for i, (ch, rate, fmt) in enumerate(formats)])
    for i in range(len(formats)):
        f.ready(i)


def test_a_round_launches_one_ingest_whatever_the_mixture_and_the_resampler_once_per_rate():
    d = lanes()
    six = timed(lambda: feed_seconds(capi.Feeder.with_formats(F.LANES, STEP), F.LANES, d["streams"], 6))
    print("launches, 6 lanes", six)
    assert set(six) == PARENT_KERNELS | {"ingest", "resample"}, six
    assert six["ingest"] == 6 and six["feeder_carry"] == 5, six
    rates = len({rate for _, rate, _ in F.LANES if rate != S.TARGET})
    assert rates == 3 and 6 <= six["resample"] <= 6 * rates, six                  # at most once per distinct rate and round
    eighteen = timed(lambda: feed_seconds(capi.Feeder.with_formats(F.LANES * 3, STEP), F.LANES * 3, d["streams"] * 3, 6))
    print("launches, 18 lanes", eighteen)
    assert eighteen == six
    # only the two 11025 Hz lanes have data: no resampler (lane 0 is copied straight, lane 1 goes through the ingest)
    two = timed(lambda: feed_seconds(capi.Feeder.with_formats(F.LANES, STEP), F.LANES, d["streams"], 6, only=(0, 1)))
    assert set(two) == PARENT_KERNELS | {"ingest"} and two["ingest"] == 6, two
    only_mono = timed(lambda: feed_seconds(capi.Feeder.with_formats(F.LANES, STEP), F.LANES, d["streams"], 6, only=(0,)))
    assert set(only_mono) == PARENT_KERNELS, only_mono
    # the uniform constructor's feeder: what the parent commit launches, no ingest
    front = {0: set(), 1: set(), 2: {"resample"}, 3: {"convert", "resample"}, 4: {"convert", "resample"}, 5: {"convert", "resample"}}
    for k, fmt in enumerate(F.LANES):
        ch, rate, sample_format = fmt
        got = timed(lambda: feed_seconds(capi.Feeder(2, ch, rate, sample_format, STEP), [fmt] * 2, [d["streams"][k]] * 2, 6, only=(0,)))
        assert set(got) == PARENT_KERNELS | front[k], (fmt, got)
    s16_surround = at_rate(signal(6 * S.TARGET, 3), 48000, 6, 1)
    got = timed(lambda: feed_seconds(capi.Feeder(1, 6, 48000, capi.SAMPLE_S16, STEP), [(6, 48000, capi.SAMPLE_S16)], [s16_surround], 6))
    assert set(got) == PARENT_KERNELS | {"downmix", "resample"}, got


# ---- 4. state ----------------------------------------------------------------------------------------------------------------------
def test_a_stereo_lane_carries_mono_state_and_the_uniform_feeder_keeps_its_stereo_tails():
    """1-s chunks of stereo s16 at 11025 Hz.  with_formats: within the mono bound of include/needle_hip.h, 76 176 B;
    needle_hip_feeder_new: above it and within its own 149 888 B.  Neither grows with the stream.  state_bytes is a
    high-water mark, and the tail a round carries depends on where keep_frame (a multiple of 4 frames = 5460 samples)
    stands in the second: 11025 mod 5460 = 105 samples a second, so the carried tail repeats every 52 chunks and the
    high-water is complete only after 52 s.  A checkpoint at 10 s is therefore below it (printed, and asserted not to
    exceed the later ones); the figures at 60 s and at 120 s, both past the period, must be EQUAL, as
    tests/test_gpu_feeder_audit.py compares its checkpoints."""
    fmt = (2, S.TARGET, capi.SAMPLE_S16)
    chunk = at_rate(signal(S.TARGET, 80), S.TARGET, 2, 1)
    a, b = capi.Feeder.with_formats([fmt], STEP), capi.Feeder(1, 2, S.TARGET, capi.SAMPLE_S16, STEP)
    state = {}
    for sec in range(120):
        a.feed([chunk])
        b.feed([chunk])
        if sec + 1 in (10, 60, 120):
            state[sec + 1] = (a.state_bytes()[0], b.state_bytes()[0])
    print("state bytes (with_formats, uniform)", state)
    assert a.items(0).tolist() == b.items(0).tolist() and a.ready(0)[0] > 400
    assert 19 * 1365 * 2 < state[60][0] <= S.STATE_BOUND[(S.TARGET, 1)] < state[60][1] <= S.STATE_BOUND[(S.TARGET, 2)], state
    assert state[60] == state[120], state
    assert state[10][0] <= state[60][0] and state[10][1] <= state[60][1], state


# ---- 5. reset_format -----------------------------------------------------------------------------------------------------------------
def test_a_lane_takes_another_format_with_its_next_stream_while_its_neighbours_hold_state():
    d = lanes()
    formats = list(F.LANES)
    f = capi.Feeder.with_formats(formats, STEP)
    seconds = [fr // fmt[1] + 1 for fr, fmt in zip(d["frames"], formats)]
    at = 8                                                                          # lane 2 (stereo s16, 44.1 kHz) is reset after 8 of 27 s
    new = F.LANES[3]                                                                # ... to six planar-float channels at 48 kHz
    rounds = [[min(fmt[1], max(fr - sec * fmt[1], 0)) for fr, fmt in zip(d["frames"], formats)] for sec in range(max(seconds))]
    second = [min(new[1], max(d["frames"][3] - sec * new[1], 0)) for sec in range(seconds[3])]
    total = max(len(rounds), at + 1 + len(second))
    rounds += [[0] * 6 for _ in range(total - len(rounds))]
    for r in range(at + 1, total):
        rounds[r][2] = second[r - at - 1] if r - at - 1 < len(second) else 0
    finishes = [[i for i in range(6) if i != 2 and seconds[i] - 1 == r] for r in range(total)]
    finishes[at + len(second)].append(2)
    first_part = []

    def reset(r, st):
        if r != at:
            return
        assert not any(st["finished"]) and all(f.ready(i)[0] > 0 for i in range(6))  # the neighbours hold tails and rows
        first_part.append(st["seen"][2])
        f.reset_format([2], [new])
        assert f.lane_format(2) == new and f.ready(2) == (0, 0, False) and len(f.items(2)) == 0
        st["streams"][2], st["formats"][2], st["pos"][2], st["seen"][2] = d["streams"][3], new, 0, np.zeros(0, dtype=np.uint32)
    items = feed_mixed(f, formats, d["streams"], (rounds, finishes), after_round=reset)
    assert len(first_part[0]) > 3 and first_part[0].tolist() == d["want"][2][: len(first_part[0])].tolist()
    assert items[2].tolist() == d["want"][3].tolist()
    for k in (0, 1, 3, 4, 5):
        assert items[k].tolist() == d["want"][k].tolist(), k


def test_reset_format_is_refused_by_a_uniform_feeder_and_changes_nothing():
    d = lanes()
    ch, rate, fmt = F.LANES[2]
    g = capi.Feeder(2, ch, rate, fmt, STEP)
    half = d["frames"][2] // 2
    g.feed([chunk_of(d["streams"][2], ch, fmt, 0, half), None])
    before = (g.ready(0), g.items(0).tolist(), g.state_bytes())
    for lane in (0, 1):
        with pytest.raises(capi.NeedleError) as e:
            g.reset_format([lane], [(1, 11025, capi.SAMPLE_S16)])
        assert e.value.name == "InvalidArgument"
    assert (g.ready(0), g.items(0).tolist(), g.state_bytes()) == before and g.lane_format(0) == F.LANES[2] == g.lane_format(1)
    g.feed([chunk_of(d["streams"][2], ch, fmt, half, d["frames"][2] - half), None])
    g.finish()
    assert g.items(0).tolist() == d["want"][2].tolist()


# ---- 6. the audit ----------------------------------------------------------------------------------------------------------------------
def test_the_audit_of_every_lane_equals_a_uniform_feeder_s_over_the_same_stream():
    d = lanes()
    f = capi.Feeder.with_formats(F.LANES, STEP)
    f.set_audit(True)
    schedule = F.mixed_schedule(d["frames"])

    def audited(r, st):
        for i in range(f.lanes):
            a = f.audit(i)
            assert a["items"] == f.ready(i)[0] and a["mismatches"] == 0 and a["accepted_mismatches"] == 0, (r, i, a)
    items = feed_mixed(f, F.LANES, d["streams"], schedule, after_round=audited)
    for k, (ch, rate, fmt) in enumerate(F.LANES):
        assert items[k].tolist() == d["want"][k].tolist(), k
        g = capi.Feeder(1, ch, rate, fmt, STEP)
        g.set_audit(True)
        g.feed([d["streams"][k]])
        g.finish()
        assert g.items(0).tolist() == items[k].tolist()
        assert f.audit(k) == g.audit(0), (k, f.audit(k), g.audit(0))
        assert f.audit(k)["items"] == len(items[k]) and f.audit(k)["accepted"] > 0


# ---- 7. a mixed season into the search -----------------------------------------------------------------------------------------------
SEASON = [(2, 48000, capi.SAMPLE_S16), (1, 11025, capi.SAMPLE_S16), (2, 44100, capi.SAMPLE_S32), (6, 48000, capi.SAMPLE_F32P)]


@pytest.fixture(scope="module")
def season():
    """Four episodes with a shared intro and outro, each in a format of its own; per video the opening and ending windows
    as the analyzer cuts them, the one-shot FrameHashes, the oracle's, and the oracle's search results."""
    eps = synth.make_library(4, 90.0, 20.0, outro_s=15.0)
    lanes_, formats, seeks, ref, one, keep = [], [], [], [], [], []
    for v, (e, fmt) in enumerate(zip(eps, SEASON)):
        ch, rate, sample_format = fmt
        s16 = e.pcm if (ch, rate) == (1, S.TARGET) else at_rate(e.pcm, rate, ch, v)
        x = in_format(s16, sample_format, 60 + v)
        ref.append(oracle_frame_hashes(convert_spec(x, ch, sample_format % 5), ch, rate))
        (o0, on), (e0, en, seek) = windows(len(x), ch, rate)
        lanes_ += [stream_of(x[ch * o0: ch * (o0 + on)], ch, sample_format), stream_of(x[ch * e0: ch * (e0 + en)], ch, sample_format)]
        formats += [fmt, fmt]
        seeks.append(seek)
        an = capi.Analyzer([f"ep{v}.wav"], include_endings=True)
        one.append(an.run_pcm([stream_of(x, ch, sample_format)], channels=ch, sample_rate=rate, hash_duration=HASH_DURATION[STEP],
                              sample_format=sample_format)[0])
        keep.append(an)
    want = O.run_with_frame_hashes(O.Comparator(include_endings=True, min_opening_duration=10 * NS, min_ending_duration=10 * NS), ref)
    assert sum(w is not None and w.opening is not None for w in want) >= 3
    return dict(lanes=lanes_, formats=formats, seeks=seeks, ref=ref, one=one, want=want, keep=keep)


def test_a_season_of_four_formats_fed_out_of_step_into_a_crossmatcher_with_regions(season):
    videos, t, min_len = 4, 10, (30, 25)
    lanes_, formats = season["lanes"], season["formats"]
    n = len(lanes_)
    frames = [(sum(len(p) for p in x) if capi.sample_format_planar(fmt[2]) else len(x)) // fmt[0] for x, fmt in zip(lanes_, formats)]
    schedule = F.mixed_schedule(frames, formats, seed=4)
    F.check_mixed_conditions(schedule, frames)
    f = capi.Feeder.with_formats(formats, STEP)
    cap = [max(capi.feeder_num_ready(frames[k], formats[k][1], formats[k][0], STEP, True) for k in range(r, n, 2)) for r in range(2)]
    m = capi.CrossMatcher.with_regions(videos, cap, min_len, t)

    def search(r, st):
        m.feed_from_feeder(f)
        assert [m.lane(k) for k in range(n)] == [(len(st["seen"][k]), st["finished"][k]) for k in range(n)], r
    items = feed_mixed(f, formats, lanes_, schedule, after_round=search)
    assert m.ready()[1]
    runs = m.runs()
    assert by_pair(runs) == regions_one_shot(items, videos, t, min_len)
    fhs = [f.frame_hashes(2 * v, 2 * v + 1, season["seeks"][v], hash_duration=HASH_DURATION[STEP]) for v in range(videos)]
    for v in range(videos):
        assert hashes_of(fhs[v]) == hashes_of(season["one"][v]) == oracle_hashes(season["ref"][v]), v
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(videos)], include_endings=True, min_opening_duration=10, min_ending_duration=10)
    got = results(cmp.results_from_runs(fhs, runs))
    assert got == results(cmp.run_with_frame_hashes(season["one"])) == results(season["want"])
