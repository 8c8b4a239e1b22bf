"""Ragged feeds for the streaming fingerprinter's tests: a deterministic schedule builder, a Python restatement of the
per-lane host arithmetic of needle_amd/csrc/feeder.hip, and the conditions C1-C6 a schedule must meet so that the lanes
of one round really differ from each other.  No device, and of the library only needle_hip_feeder_num_ready (through
which the restatement is checked, tests/test_feeder_ragged_cpu.py).

A schedule is (rounds, finishes): rounds[r][i] is the number of frames (samples per channel at the source rate) lane i
is given in feed r; finishes[r] lists the lanes that get `finish` after feed r."""
from collections import namedtuple
from math import gcd

import numpy as np

from needle_amd import capi
from oracle import oracle as O

HOP, FRAME, LATENCY, TARGET = 1365, 4096, 19, 11025
# include/needle_hip.h: the resampler's tile in outputs, by rate
TILE = {44100: 1280, 22050: 1536, 48000: 2352, 96000: 2352, 32000: 7056, 12345: 11760}
# the documented bound of needle_hip_feeder_state_bytes()[0], by (rate, channels)
STATE_BOUND = {(11025, 1): 76_176, (11025, 2): 149_888, (48000, 2): 117_760}

Config = namedtuple("Config", "rate ch fmt step seconds seed")
# tests/test_gpu_feeder_ragged.py's configurations; `a` runs at steps 1, 2 and 3.  The seeds are ones whose schedule meets
# C1-C6 (tests/test_feeder_ragged_cpu.py asserts it): with three or four lanes not every seed puts a lane of each kind
# into one round.
CONFIGS = {
    "a1": Config(11025, 1, capi.SAMPLE_S16, 1, (30, 14, 0.2, 0, 22, 9), 1),
    "a2": Config(11025, 1, capi.SAMPLE_S16, 2, (30, 14, 0.2, 0, 22, 9), 1),
    "a3": Config(11025, 1, capi.SAMPLE_S16, 3, (30, 14, 0.2, 0, 22, 9), 1),
    "b": Config(11025, 2, capi.SAMPLE_S16, 2, (20, 11, 6, 15), 2),
    "c": Config(48000, 2, capi.SAMPLE_S16, 2, (16, 9, 0.1, 12, 5), 3),
    "d": Config(44100, 2, capi.SAMPLE_S32, 3, (12, 7, 10, 3), 18),
    "e": Config(12345, 1, capi.SAMPLE_S16, 2, (25, 12, 18), 15),
    "f": Config(48000, 6, capi.SAMPLE_F32P, 2, (10, 6, 8, 2), 5),
    "g": Config(11025, 2, capi.SAMPLE_F64, 1, (8, 5, 3), 5),
}


def whole_stream_window(frames, rate):
    """Frames of the analyzer's opening window with the search percentage at 1.0 (tests/test_gpu_feeder.py's): what
    Analyzer.run_pcm fingerprints of a stream of `frames`."""
    dur = O.duration_from_secs_f64(frames * (1.0 / rate))
    return min(O.duration_mul_f32(dur, 1.0) * rate // O.NS, frames)


def config_frames(cfg):
    """Source frames of every lane: `seconds` of 11025 Hz content brought to the rate (at_rate's length), cut to the
    analyzer's whole-stream window."""
    return [whole_stream_window(int(int(round(s * TARGET)) * cfg.rate / TARGET), cfg.rate) for s in cfg.seconds]


# ---- the lane arithmetic, restated ---------------------------------------------------------------------------------
def tiling(rate):
    """(L, M, half, T): outputs per M inputs, the filter's half length in inputs, the tile in outputs."""
    g = gcd(TARGET, rate)
    L, M = TARGET // g, rate // g
    half = -(-16 * M // L) if M > L else 16
    return L, M, half, TILE[rate]


def final_outputs(fed, rate):
    """(tiles, outputs) of an unfinished stream's first `fed` frames: whole tiles whose taps lie inside them."""
    if rate == TARGET:
        return 0, fed
    L, M, half, T = tiling(rate)
    avail = -(-(fed - half) * L // M) if fed > half else 0
    return avail // T, avail // T * T


Lane = namedtuple("Lane", "fed raw frames kept keep_frame skew tiles outputs carried src_tail")


def mirror(fed, rate, ch, step):
    """An unfinished lane after `fed` source frames, however they were cut.  `frames` is raw + 19 where there is a raw
    item; inside the latency it is the even number of whole frames of the outputs.  `carried`: the s16 values of the
    11025 Hz tail the next round's carry moves; `src_tail`: the source frames it moves (other rates)."""
    raw = capi.feeder_num_ready(fed, rate, ch, 1, False)
    tiles, outputs = final_outputs(fed, rate)
    frames = raw + LATENCY if raw > 0 else (0 if outputs < FRAME else (outputs - FRAME) // HOP + 1) & ~1
    kept = -(-raw // step)
    keep_frame = min(kept * step, frames) & ~3
    pcm_channels = 1 if rate != TARGET else min(ch, 2)
    skew = keep_frame * HOP * pcm_channels % 8
    src_tail = 0
    if rate != TARGET:
        L, M, half, T = tiling(rate)
        first = tiles * T * M // L - half + 1
        src_tail = fed - min(max(first, 0) & ~7, fed & ~7)
    return Lane(fed, raw, frames, kept, keep_frame, skew, tiles, outputs, (outputs - keep_frame * HOP) * pcm_channels, src_tail)


# ---- schedules -------------------------------------------------------------------------------------------------------
def _size(k, rate, rng):
    """One chunk of class k in source frames.  The classes that are lengths of OUTPUT (a hop, a frame, a tile, seconds)
    are scaled by rate / 11025; the two below eight frames are source frames as they stand.  At 11025 Hz, where there
    is no resampler tile, the tile's class is the four frames (5460 samples) `keep_frame` advances by."""
    T = TILE.get(rate, 4 * HOP)

    def src(outputs):
        return -(-outputs * rate // TARGET)
    if k == 0:
        return 0
    if k == 1:
        return int(rng.integers(1, 4))
    if k == 2:
        return int(rng.integers(5, 8))
    if k == 3:
        return src(HOP) + int(rng.integers(-1, 2))
    if k == 4:
        return src(FRAME)
    if k == 5:
        return src(T) + int(rng.choice([-1, 1])) * int(rng.integers(1, 9))
    if k == 6:
        return int(rng.integers(src(3 * T), src(5 * T) + 1))
    return int(rng.integers(2 * rate, 4 * rate + 1))


def ragged_schedule(lens, rate, seed):
    """(rounds, finishes) that feed lane i lens[i] frames in all.  Every lane waits zero to four rounds, then most open
    with chunks below eight frames and a pause after each (so a lane holds 1-7 frames over several rounds while
    others are in full flow), then draws class after class until its stream is spent; a lane that was not left out
    twice, in rounds that are not consecutive, gets pauses inserted.  A lane is finished after the round that spends it,
    a lane of no frames after the last round."""
    rng = np.random.default_rng(seed)
    cols = []
    for total in lens:
        col, left = [0] * int(rng.integers(0, 5)), int(total)
        opening = int(rng.integers(0, 3))
        if opening == 0:
            head = [int(rng.integers(1, 4)), 0, int(rng.integers(1, 4)), 0]
        elif opening == 1:
            head = [int(rng.integers(5, 8)), 0]
        else:
            head = []
        for c in head:
            c = min(c, left)
            col.append(c)
            left -= c
        while left > 0:
            c = min(_size(int(rng.integers(0, 8)), rate, rng), left)
            col.append(c)
            left -= c
        cols.append(col)
    lead = min(next((r for r, c in enumerate(col) if c), len(col)) for col, total in zip(cols, lens) if total)
    cols = [col[lead:] for col in cols]                                         # the first round feeds somebody
    for col, total in zip(cols, lens):                                          # left out twice before its last chunk
        while total:
            zeros = [r for r, c in enumerate(col) if c == 0]
            if len(zeros) >= 2 and zeros[-1] - zeros[0] >= 2:
                break
            col.insert(int(rng.integers(0, len(col))), 0)
    n_rounds = max(len(c) for c in cols)
    rounds = [[c[r] if r < len(c) else 0 for c in cols] for r in range(n_rounds)]
    finishes = [[] for _ in range(n_rounds)]
    for i, col in enumerate(cols):
        finishes[len(col) - 1 if lens[i] else n_rounds - 1].append(i)
    return rounds, finishes


def properties(schedule, rate, ch, step):
    """Per round, what its lanes do, from the mirror.  `live`: unfinished when the round begins, in lane order."""
    rounds, finishes = schedule
    n = len(rounds[0])
    fed, finished, out = [0] * n, [False] * n, []
    for chunks, done in zip(rounds, finishes):
        live = [i for i in range(n) if not finished[i]]
        before = [mirror(f, rate, ch, step) for f in fed]
        fed = [f + c for f, c in zip(fed, chunks)]
        after = [mirror(f, rate, ch, step) for f in fed]
        carrying = [i for i in live if before[i].carried > 0]
        order = {i: k for k, i in enumerate(live)}
        p = dict(chunks=chunks, live=live, before=before, after=after, finish=list(done),
                 fed=[i for i in live if chunks[i]],
                 idle=[i for i in live if not chunks[i]],
                 first_only=[i for i in live if after[i].frames > before[i].frames and after[i].kept == before[i].kept],
                 raw_only=[i for i in live if after[i].raw > before[i].raw and after[i].kept == before[i].kept],
                 second=[i for i in live if after[i].kept > before[i].kept],
                 skew={i: before[i].skew for i in carrying},
                 tiles={i: after[i].tiles - before[i].tiles for i in live},
                 small_tail=[i for i in live if 1 <= before[i].src_tail <= 7 or 1 <= after[i].src_tail <= 7],
                 holding=[i for i in live if i not in done and after[i].raw > 0])
        p["skew_neighbours"] = [(i, j) for i in carrying for j in carrying
                                if order[j] == order[i] + 1 and before[i].skew != before[j].skew]
        out.append(p)
        for i in done:
            finished[i] = True
    return out


def conditions(props, rate, ch, step):
    """{condition: the rounds that meet it} (C5, C6: the rounds they count).  C2 is stated on what puts a lane into the
    `first` table alone: new frame pairs and no new kept item.  Unfinished frames come in pairs, so raw items are odd
    in number and at step 1 and 2 every new raw item brings a kept one: there a lane is in `first` alone only inside the
    19-frame latency.  "C2raw" lists the rounds where a lane gains raw items and no kept one (step 3)."""
    c = {k: [] for k in ("C1", "C2", "C2raw", "C3", "C4", "C5one", "C6")}
    skipped = {}
    for r, p in enumerate(props):
        sizes = sorted({p["chunks"][i] for i in p["fed"]})
        if len(sizes) >= 3 and sizes[-1] >= 100 * sizes[0]:
            c["C1"].append(r)
        if p["first_only"] and p["second"] and p["idle"]:
            c["C2"].append(r)
            if p["raw_only"]:
                c["C2raw"].append(r)
        if p["skew_neighbours"]:
            c["C3"].append(r)
        many = [i for i in p["fed"] if p["tiles"][i] >= 2]
        none = [i for i in p["fed"] if p["tiles"][i] == 0]
        if any(len({i, j, k}) == 3 for i in many for j in none for k in p["small_tail"]):
            c["C4"].append(r)
        if len(p["fed"]) == 1:
            c["C5one"].append(r)
        for i in p["idle"]:
            skipped.setdefault(i, []).append(r)
        if p["finish"]:
            c["C6"].append(r)
    c["C5"] = {i: v for i, v in skipped.items()}
    c["C6held"] = [r for r in c["C6"] if props[r]["holding"]]
    return c


def check_conditions(schedule, rate, ch, step):
    """Asserts C1-C6 for the schedule and returns conditions()'s rounds."""
    props = properties(schedule, rate, ch, step)
    c = conditions(props, rate, ch, step)
    n = len(schedule[0][0])
    assert c["C1"], "C1: three chunks of different sizes, the largest 100 times the smallest, in one round"
    assert c["C2"], "C2: a lane in the first table only, one with new kept items and an idle one in one round"
    if step >= 3:
        assert c["C2raw"], "C2: ... where a lane gains raw items and no kept one"
    if rate == TARGET and ch == 1:
        assert c["C3"], "C3: skew 0 next to skew 4 in one carry"
    elif rate == TARGET:
        # two channels: keep_frame is a multiple of 4 and 4 x 1365 x 2 = 8 x 1365, so the skew is 0 for every lane in
        # every round -- there are no two skews to mix
        assert all(v == 0 for p in props for v in p["skew"].values()) and not c["C3"]
    else:
        assert c["C4"], "C4: two tiles or more, fed without a tile, and a source tail of 1-7 frames in one round"
    for i in range(n):
        gaps = c["C5"].get(i, [])
        assert len(gaps) >= 2 and gaps[-1] - gaps[0] >= 2, f"C5: lane {i} is left out in {gaps}"
    assert c["C5one"], "C5: a round fed to exactly one lane"
    assert len(c["C6"]) >= 3 and c["C6held"], "C6: finishes in three rounds, one beside lanes that hold raw items"
    return c


def feed_pieces(chunks, bound_values, ch):
    """Feeder::Feed's internal cutting under NEEDLE_HIP_MAX_BATCH_VALUES, restated: the per-lane frames of every
    internal round of one feed."""
    bound = max(bound_values // ch, 1)
    done, out = [0] * len(chunks), []
    while True:
        left, piece = bound, []
        for i, c in enumerate(chunks):
            take = min(c - done[i], left)
            piece.append(take)
            done[i] += take
            left -= take
        out.append(piece)
        if done == list(chunks):
            return out


def staging_bound(rounds, ch):
    """(NEEDLE_HIP_MAX_BATCH_VALUES, rounds) such that the largest chunk of the schedule alone is cut three times
    inside Feed; the rounds listed are the feeds in which a piece spends the bound before it reaches a later lane
    that still has frames to give."""
    bound = (max(max(r) for r in rounds) // 4 + 1) * ch
    starved = []
    for r, chunks in enumerate(rounds):
        left = list(chunks)
        for piece in feed_pieces(chunks, bound, ch):
            left = [a - b for a, b in zip(left, piece)]
            if any(piece[j] == 0 and left[j] > 0 and any(piece[:j]) for j in range(len(chunks))):
                starved.append(r)
                break
    return bound, starved


def reset_round(schedule, cfg, lane, others):
    """The first round after which `lane` has been fed a third of its stream while `others` hold raw items and are
    unfinished."""
    rounds, finishes = schedule
    total = sum(chunks[lane] for chunks in rounds)
    fed, finished = [0] * len(rounds[0]), set()
    for r, chunks in enumerate(rounds):
        fed = [f + c for f, c in zip(fed, chunks)]
        finished |= set(finishes[r])
        if fed[lane] >= total // 3 and lane not in finished and not finished & set(others) and \
                all(mirror(fed[i], cfg.rate, cfg.ch, cfg.step).raw > 0 for i in others):
            return r
    raise AssertionError("no round to reset in")


# ---- the further schedules of tests/test_gpu_feeder_ragged.py ---------------------------------------------------------
# the adversarial stream, the two hostile episodes (120 s) and an ordinary lane of 40 s, s16 mono at 11025 Hz
CONTESTED_FRAMES, CONTESTED_SEED = [634_740, 1_323_000, 1_323_000, 441_000], 0
# five episodes of 90 s at 48 kHz stereo: opening and ending windows (ten lanes), or the opening windows alone (five)
CHAIN_RATE, CHAIN_CH, CHAIN_STEP, CHAIN_MONO_FRAMES, CHAIN_SEED, OPENINGS_SEED = 48000, 2, 2, 992_250, 0, 0


def chain_frames(endings=True):
    """Frames of the lanes cut from five such episodes as the analyzer cuts its windows: lane 2v the opening window of
    video v and lane 2v + 1 its ending window, or lane v the opening window alone."""
    from tests.test_gpu_library_rates import windows
    frames = int(CHAIN_MONO_FRAMES * CHAIN_RATE / TARGET)
    (_, n_open), (_, n_end, _) = windows(frames * CHAIN_CH, CHAIN_CH, CHAIN_RATE)
    return [n_open, n_end] * 5 if endings else [n_open] * 5
