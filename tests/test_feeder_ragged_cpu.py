"""The ragged feeds of tests/test_gpu_feeder_ragged.py without a device: every configuration's schedule meets the
conditions C1-C6 that make its lanes differ inside one round (tests/feeder_schedules.py), and the restated lane
arithmetic equals needle_hip_feeder_num_ready at every (lane, round)."""
import pytest

from needle_amd import capi
from tests import feeder_schedules as S


@pytest.fixture(scope="module", params=sorted(S.CONFIGS))
def case(request):
    cfg = S.CONFIGS[request.param]
    lens = S.config_frames(cfg)
    return cfg, lens, S.ragged_schedule(lens, cfg.rate, cfg.seed)


def test_the_schedule_feeds_every_lane_its_stream_and_is_deterministic(case):
    cfg, lens, (rounds, finishes) = case
    assert [sum(r[i] for r in rounds) for i in range(len(lens))] == lens
    assert sorted(i for done in finishes for i in done) == list(range(len(lens)))
    for i, n in enumerate(lens):                                                # finished with the chunk that spends it
        last = max([r for r, chunks in enumerate(rounds) if chunks[i]], default=len(rounds) - 1)
        assert i in finishes[last] or (n == 0 and i in finishes[-1])
    assert S.ragged_schedule(lens, cfg.rate, cfg.seed) == (rounds, finishes)
    assert S.ragged_schedule(lens, cfg.rate, cfg.seed + 100) != (rounds, finishes)
    assert all(min(r) >= 0 for r in rounds) and len(rounds) < 200


def test_conditions_c1_to_c6(case):
    cfg, lens, schedule = case
    c = S.check_conditions(schedule, cfg.rate, cfg.ch, cfg.step)
    print({k: v[:4] if isinstance(v, list) else v for k, v in c.items() if k != "C5"})


def test_the_mirror_equals_the_library_at_every_lane_and_round(case):
    cfg, lens, (rounds, finishes) = case
    fed = [0] * len(lens)
    for chunks in rounds:
        fed = [f + c for f, c in zip(fed, chunks)]
        for f in fed:
            m = S.mirror(f, cfg.rate, cfg.ch, cfg.step)
            assert m.kept == capi.feeder_num_ready(f, cfg.rate, cfg.ch, cfg.step, False), (f, m)
            assert m.raw == max(m.frames - S.LATENCY, 0) and m.frames % 2 == 0 and m.keep_frame % 4 == 0, (f, m)
            assert 0 <= m.keep_frame <= min(m.kept * cfg.step, m.frames) and m.carried >= 0 and 0 <= m.src_tail <= f, (f, m)
            if m.raw:
                assert m.frames == m.raw + S.LATENCY
    L = capi.lib()
    for f in fed:                                                               # finished: the one-shot's count
        out = int(L.needle_hip_resample_out_len(f, cfg.rate)) if cfg.rate != S.TARGET else f
        want = int(L.needle_hip_fingerprint_num_kept(out, cfg.step))
        assert capi.feeder_num_ready(f, cfg.rate, cfg.ch, cfg.step, True) == want
        frames = 0 if out < S.FRAME else (out - S.FRAME) // S.HOP + 1
        assert want == -(-max(frames - S.LATENCY, 0) // cfg.step)
    assert fed == lens


@pytest.mark.parametrize("rate", sorted(S.TILE))
def test_the_mirror_s_tiles_step_with_the_library_s_count(rate):
    """Over a sweep of stream lengths: the raw count is the whole frame pairs of the mirror's whole tiles."""
    n = 0
    while n < 6 * rate:
        tiles, outputs = S.final_outputs(n, rate)
        frames = (0 if outputs < S.FRAME else (outputs - S.FRAME) // S.HOP + 1) & ~1
        assert capi.feeder_num_ready(n, rate, 1, 1, False) == max(frames - S.LATENCY, 0), (rate, n)
        assert outputs == tiles * S.TILE[rate]
        n += 1 if n < 3000 else 37
    assert S.final_outputs(6 * rate, rate)[0] >= 2


@pytest.mark.parametrize("name", ["a2", "c"])
def test_the_staging_bound_is_spent_before_the_last_lane(name):
    cfg = S.CONFIGS[name]
    rounds, _ = S.ragged_schedule(S.config_frames(cfg), cfg.rate, cfg.seed)
    bound, starved = S.staging_bound(rounds, cfg.ch)
    largest = max(max(r) for r in rounds)
    pieces = S.feed_pieces([largest], bound, cfg.ch)
    assert len(pieces) >= 4, "the largest chunk is cut at least three times"
    assert starved, "some feed spends the bound before it reaches its last lane with a chunk"


def test_the_reset_point_of_configuration_a(case):
    cfg, lens, schedule = case
    if cfg != S.CONFIGS["a2"]:
        return
    r = S.reset_round(schedule, cfg, lane=1, others=(0, 4))
    fed = sum(chunks[1] for chunks in schedule[0][: r + 1])
    assert lens[1] // 3 <= fed < lens[1] and r + 1 < len(schedule[0])


@pytest.mark.parametrize("which", ["contested-2", "contested-3", "chain", "openings"])
def test_the_further_schedules_meet_the_conditions_too(which):
    if which.startswith("contested"):
        lens, rate, ch, step, seed = S.CONTESTED_FRAMES, S.TARGET, 1, int(which[-1]), S.CONTESTED_SEED
    else:
        lens, rate, ch, step = S.chain_frames(which == "chain"), S.CHAIN_RATE, S.CHAIN_CH, S.CHAIN_STEP
        seed = S.CHAIN_SEED if which == "chain" else S.OPENINGS_SEED
    rounds, finishes = S.ragged_schedule(lens, rate, seed)
    assert [sum(r[i] for r in rounds) for i in range(len(lens))] == lens
    S.check_conditions((rounds, finishes), rate, ch, step)
    fed = [0] * len(lens)
    for chunks in rounds:
        fed = [f + c for f, c in zip(fed, chunks)]
        for f in fed:
            assert S.mirror(f, rate, ch, step).kept == capi.feeder_num_ready(f, rate, ch, step, False)
