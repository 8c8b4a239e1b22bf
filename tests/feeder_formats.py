"""Lanes that differ in rate, channel count and sample format, for the tests of Feeder.with_formats: the six lanes, a
ragged schedule over them built lane by lane with tests/feeder_schedules.py (every lane's chunk classes are scaled to its
own rate), and the conditions that schedule must meet.  No device."""
from needle_amd import capi
from tests import feeder_schedules as S

STEP = 2
# (channels, rate, format) and the seconds of 11025 Hz content behind each lane
LANES = [(1, 11025, capi.SAMPLE_S16), (2, 11025, capi.SAMPLE_S16), (2, 44100, capi.SAMPLE_S16),
         (6, 48000, capi.SAMPLE_F32P), (1, 48000, capi.SAMPLE_U8), (2, 22050, capi.SAMPLE_S32)]
SECONDS = [24, 20, 27, 22, 30, 25]
SEED = 3


def lane_config(k, lanes=LANES, seconds=SECONDS):
    """Lane k as a one-lane configuration of tests/feeder_schedules.py (and of tests/test_gpu_feeder_ragged.py's content)."""
    ch, rate, fmt = lanes[k]
    return S.Config(rate, ch, fmt, STEP, (seconds[k],), 100 + k)


def lane_frames(lanes=LANES, seconds=SECONDS):
    return [S.config_frames(lane_config(k, lanes, seconds))[0] for k in range(len(lanes))]


def mixed_schedule(frames, lanes=LANES, seed=SEED):
    """(rounds, finishes) over lanes of different rates: lane i's column is ragged_schedule's for that lane alone at its
    own rate, started `i % 3` rounds late; then, round by round, where more than one lane is still unfinished and every
    one of them has a chunk, one of them (in rotation) waits a round.  A lane is finished after the round that spends
    it."""
    cols = []
    for i, (n, (_, rate, _)) in enumerate(zip(frames, lanes)):
        rounds, _ = S.ragged_schedule([n], rate, seed + 17 * i)
        cols.append([0] * (i % 3) + [r[0] for r in rounds])
    r = 0
    while r < max(len(c) for c in cols):
        live = [i for i, c in enumerate(cols) if len(c) > r]
        if len(live) > 1 and all(cols[i][r] for i in live):
            cols[live[r % len(live)]].insert(r, 0)
        r += 1
    n_rounds = max(len(c) for c in cols)
    rounds = [[c[r] if r < len(c) else 0 for c in cols] for r in range(n_rounds)]
    finishes = [[i for i, c in enumerate(cols) if len(c) - 1 == r] for r in range(n_rounds)]
    return rounds, finishes


def check_mixed_conditions(schedule, frames):
    """An idle unfinished lane in EVERY round in which more than one lane is unfinished (and every lane idle in some round
    before its last chunk), chunks 100:1 in one round, finishes in three different rounds."""
    rounds, finishes = schedule
    n = len(frames)
    assert [sum(r[i] for r in rounds) for i in range(n)] == list(frames)
    assert sorted(i for done in finishes for i in done) == list(range(n))
    finished, idle_rounds, idle_lanes, ratio = set(), 0, set(), []
    for r, (chunks, done) in enumerate(zip(rounds, finishes)):
        live = [i for i in range(n) if i not in finished]
        fed = [i for i in live if chunks[i]]
        idle = [i for i in live if not chunks[i]]
        assert idle or len(live) <= 1, f"round {r}: no idle lane among {live}"
        if fed and idle:
            idle_rounds += 1
            idle_lanes |= set(idle)
        sizes = sorted(chunks[i] for i in fed)
        if len(sizes) >= 3 and sizes[-1] >= 100 * sizes[0]:
            ratio.append(r)
        finished |= set(done)
    assert idle_lanes == set(range(n)), idle_lanes
    assert ratio, "three chunks of different sizes, the largest 100 times the smallest, in one round"
    assert len([r for r, done in enumerate(finishes) if done]) >= 3, "finishes in three different rounds"
    return dict(idle_rounds=idle_rounds, rounds=len(rounds), ratio=ratio)
