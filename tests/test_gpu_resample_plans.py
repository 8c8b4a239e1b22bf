"""-m gpu: the resampler at every kernel plan a rate can select.  tests/resample_plans.py's table holds a rate of every
class of plan (tests/test_resample_plan_cpu.py proves it by a sweep of the planner over all rates); each case first
asserts from needle_hip_resample_plan which plan its rate takes, so a failure names the kernel and its geometry, then
compares needle_hip_resample_host with oracle/ora_resample.c for exact equality.  Then the plans only the tuning switches
reach, persistent matrix-core workgroups on the plans with few blocks, unaligned and pieced library PCM on the layouts
no library test had met, and a mixed feeder over four of the new rates."""
import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests import feeder_formats as F
from tests import resample_plans as P

pytestmark = pytest.mark.gpu
SWITCHES = ("NEEDLE_HIP_RESAMPLE_V1", "NEEDLE_HIP_RESAMPLE_QUAD", "NEEDLE_HIP_RESAMPLE_SPLITS", "NEEDLE_HIP_RESAMPLE_GRID",
            "NEEDLE_HIP_RESAMPLE_LAYOUT")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


@pytest.fixture(autouse=True)
def _default_environment(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


_REFERENCE = {}


def reference(rate, ch, lens, plan):
    """The streams of a case and the oracle's outputs, made once per (rate, channels, lengths) and never changed; the
    conditions on the inputs are checked here, on the oracle's output alone."""
    key = (rate, ch, tuple(lens))
    if key not in _REFERENCE:
        pcms = [P.signal(n, ch, plan, 10 * k + ch) for k, n in enumerate(lens)]
        want = [O.resample(x, ch, rate) for x in pcms]
        for x, w, n in zip(pcms, want, lens):
            assert len(w) == capi.lib().needle_hip_resample_out_len(n, rate)
            P.check_reference(w, n, plan)
            x.setflags(write=False)
        _REFERENCE[key] = (pcms, [w.tolist() for w in want])
    return _REFERENCE[key]


def assert_equals_the_oracle(rate, ch, lens, plan, what):
    pcms, want = reference(rate, ch, lens, plan)
    got = capi.resample(pcms, ch, rate)
    for k, (g, w) in enumerate(zip(got, want)):
        if g.tolist() != w:
            g, w = np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64)
            bad = np.nonzero(g != w)[0] if len(g) == len(w) else []
            raise AssertionError(f"{what}: stream {k} of {lens[k]} samples differs from the oracle at {len(bad)} of {len(w)} "
                                 f"outputs, first at {bad[:8].tolist()} (tile {plan['tile_outputs']}, L {plan['L']})")


# ---- 1. every class of plan -----------------------------------------------------------------------------------------------------
def _case_id(rate):
    return f"{rate}"


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate", P.RATES, ids=_case_id)
def test_plan_equals_the_oracle(rate, ch):
    plan = capi.resample_plan(rate)
    key = P.class_key(plan)
    assert key == CLASS_OF[rate], (rate, key)
    print(rate, ch, " ".join(key), {k: v for k, v in plan.items() if v and k != "family"})
    assert_equals_the_oracle(rate, ch, P.stream_lengths(plan), plan, f"{rate} Hz x{ch} {' '.join(key)}")


# The class each rate of the table takes, written out: a planner change that moves a rate to another kernel fails the
# case that no longer runs what it says (and the CPU test fails if a class is then left without a rate).
_G, _M, _Q = "general", "mfma", "quad"
CLASS_OF = {
    44100: ("dec", "q5"), 22050: ("dec", "q6"), 11025: ("identity",),
    2205: (_G, "contiguous", "global", "scalar", "n1024"), 2835: (_G, "contiguous", "global", "scalar", "n128"),
    2030: (_G, "contiguous", "global", "scalar", "n16"), 3675: (_G, "contiguous", "global", "scalar", "n2048"),
    2625: (_G, "contiguous", "global", "scalar", "n256"), 2175: (_G, "contiguous", "global", "scalar", "n32"),
    33075: (_G, "contiguous", "global", "scalar", "n4096"), 2450: (_G, "contiguous", "global", "scalar", "n512"),
    2058: (_G, "contiguous", "global", "scalar", "n64"), 7350: (_G, "contiguous", "global", "scalar", "n2048"),
    543900: (_G, "contiguous", "global", "vec4", "n128"), 617400: (_G, "contiguous", "global", "vec4", "n256"),
    529200: (_G, "contiguous", "global", "vec4", "n512"), 714420: (_G, "contiguous", "global", "vec4", "n64"),
    705600: (_G, "contiguous", "global", "vec4", "n256"),
    8820: (_G, "contiguous", "rows-in-lds", "vec4", "n1024"), 2520: (_G, "contiguous", "rows-in-lds", "vec4", "n128"),
    14700: (_G, "contiguous", "rows-in-lds", "vec4", "n2048"), 2100: (_G, "contiguous", "rows-in-lds", "vec4", "n256"),
    2400: (_G, "contiguous", "rows-in-lds", "vec4", "n32"), 4900: (_G, "contiguous", "rows-in-lds", "vec4", "n512"),
    2352: (_G, "contiguous", "rows-in-lds", "vec4", "n64"), 352800: (_G, "contiguous", "rows-in-lds", "vec4", "n512"),
    37800: (_G, "contiguous", "rows-in-lds", "vec4", "n1024"),
    642929: (_G, "row", "global", "scalar", "n1"), 602070: (_G, "row", "global", "scalar", "n2"),
    721917: (_G, "row", "global", "scalar", "n4"), 713475: (_G, "row", "global", "scalar", "n8"),
    643076: (_G, "row", "global", "vec4", "n1"), 603120: (_G, "row", "global", "vec4", "n2"),
    721476: (_G, "row", "global", "vec4", "n4"), 718200: (_G, "row", "global", "vec4", "n8"),
    384000: (_G, "row", "global", "vec4", "n4"),
    4800: (_M, "steps12", "rows-fit", "splits1", "waves10"), 9408: (_M, "steps12", "rows-fit", "splits1", "waves<10"),
    2240: (_M, "steps12", "rows-fit", "splits2", "waves10"), 4032: (_M, "steps12", "rows-fit", "splits2", "waves<10"),
    2000: (_M, "steps12", "rows-fit", "splits>=3", "waves10"), 2184: (_M, "steps12", "rows-fit", "splits>=3", "waves<10"),
    11024: (_M, "steps12", "rows-fit", "splits>=3", "waves10"),
    11100: (_M, "steps20", "rows-fit", "splits1", "waves10"), 14400: (_M, "steps20", "rows-fit", "splits1", "waves<10"),
    11060: (_M, "steps20", "rows-fit", "splits2", "waves10"), 11088: (_M, "steps20", "rows-fit", "splits2", "waves<10"),
    11300: (_M, "steps20", "rows-fit", "splits>=3", "waves10"), 11256: (_M, "steps20", "rows-fit", "splits>=3", "waves<10"),
    19200: (_M, "steps36", "rows-fit", "splits1", "waves10"), 28224: (_M, "steps36", "rows-fit", "splits1", "waves<10"),
    18760: (_M, "steps36", "rows-fit", "splits2", "waves10"), 18648: (_M, "steps36", "rows-fit", "splits2", "waves<10"),
    18700: (_M, "steps36", "rows-fit", "splits>=3", "waves10"), 18732: (_M, "steps36", "rows-fit", "splits>=3", "waves<10"),
    29896: (_M, "steps36", "rows-fit", "splits>=3", "waves10"),
    33900: (_M, "steps52", "rows-fit", "splits1", "waves10"), 35700: (_M, "steps52", "rows-fit", "splits1", "waves<10"),
    33880: (_M, "steps52", "rows-fit", "splits2", "waves10"), 33768: (_M, "steps52", "rows-fit", "splits2", "waves<10"),
    33800: (_M, "steps52", "rows-fit", "splits>=3", "waves10"), 33852: (_M, "steps52", "rows-fit", "splits>=3", "waves<10"),
    36300: (_M, "steps52", "long-row", "splits1", "waves10"),
    102375: (_Q, "scalar", "small", "splits1", "rounds1"), 9849: (_Q, "scalar", "small", "splits2", "rounds1"),
    4875: (_Q, "scalar", "small", "splits>=3", "rounds1"), 22254: (_Q, "scalar", "small", "splits>=3", "rounds1"),
    141120: (_Q, "vec4", "small", "splits1", "rounds1"), 48804: (_Q, "vec4", "small", "splits2", "rounds1"),
    48900: (_Q, "vec4", "small", "splits>=3", "rounds1"), 64000: (_Q, "vec4", "small", "splits>=3", "rounds1"),
    50000: (_Q, "vec4", "small", "splits>=3", "rounds1"), 47952: (_Q, "vec4", "small", "splits>=3", "rounds1"),
}
assert sorted(CLASS_OF) == sorted(P.RATES)


# ---- 2. persistent matrix-core workgroups on the plans with few blocks ----------------------------------------------------------
@pytest.mark.parametrize("rate,ch,splits,waves,steps", [(2240, 2, 2, 10, 12), (9408, 1, 1, 5, 12), (33900, 2, 1, 10, 52),
                                                        (33768, 1, 2, 6, 52)])
def test_three_persistent_workgroups_walk_many_tiles(monkeypatch, rate, ch, splits, waves, steps):
    """NEEDLE_HIP_RESAMPLE_GRID=3: a few workgroups do the work of dozens, so the steady state (a tile written to LDS while
    the next one's loads replace it in the registers) runs on the plans with a tile cut in two, with waves that have no
    block, and in the 52-step kernel with rows that fit."""
    plan = capi.resample_plan(rate)
    assert plan["family"] == "mfma" and plan["mf_long_row"] == 0
    assert (plan["mf_splits"], plan["mf_waves"], plan["mfma_steps"]) == (splits, waves, steps)
    if (splits, waves) == (2, 6):
        assert plan["nblocks"] < 2 * waves                          # the second workgroup of a tile holds fewer blocks
    tile_in = plan["tile_outputs"] // plan["L"] * plan["M"]
    lens = [23 * tile_in + 5, 0, 9 * tile_in, plan["T"] // 2 - 1, 14 * tile_in + plan["M"] // 2 + 3]
    monkeypatch.setenv("NEEDLE_HIP_RESAMPLE_GRID", "3")
    assert_equals_the_oracle(rate, ch, lens, plan, f"{rate} Hz x{ch} three persistent workgroups")


# ---- 3. the plans only a switch reaches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate,env,want", [
    # <CH, false, false>, two rounds, a tile cut in two
    (12345, {"SPLITS": "2"}, dict(vec4=0, quad_small=0, quad_threads=1024, quad_rounds=2, quad_splits=2)),
    # <CH, true, false>, two rounds, one workgroup per tile (an 8 kHz tile otherwise goes to the matrix cores)
    (8000, {"SPLITS": "1", "QUAD": "1"}, dict(vec4=1, quad_small=0, quad_threads=1024, quad_rounds=2, quad_splits=1)),
    (12345, {"SPLITS": "4"}, dict(vec4=0, quad_small=0, quad_threads=768, quad_rounds=1, quad_splits=4)),
    (64000, {"SPLITS": "2"}, dict(vec4=1, quad_small=0, quad_threads=896, quad_rounds=1, quad_splits=2)),
], ids=["12345-2splits", "8000-1split", "12345-4splits", "64000-2splits"])
def test_quad_kernel_for_large_workgroups_and_two_rounds(monkeypatch, rate, env, want, ch):
    """NEEDLE_HIP_RESAMPLE_SPLITS is the only way to the instantiations for more than 640 threads and to a second round
    of quads (kQuadMaxRounds)."""
    for k, v in env.items():
        monkeypatch.setenv("NEEDLE_HIP_RESAMPLE_" + k, v)
    plan = capi.resample_plan(rate)
    assert plan["family"] == "quad" and {k: plan[k] for k in want} == want, plan
    assert_equals_the_oracle(rate, ch, P.stream_lengths(plan), plan, f"{rate} Hz x{ch} quad, {env}")


@pytest.mark.parametrize("ch", [1, 2])
def test_general_kernel_with_rows_in_lds_and_scalar_staging(monkeypatch, ch):
    """NEEDLE_HIP_RESAMPLE_V1 on a row-layout rate with M % 4 != 0: resample_kernel<CH, true, false>, which no rate takes
    by default (the quad kernel has them all)."""
    monkeypatch.setenv("NEEDLE_HIP_RESAMPLE_V1", "1")
    plan = capi.resample_plan(12345)
    assert P.class_key(plan) == ("general", "row", "rows-in-lds", "scalar", "n16") and plan["M"] % 4 != 0
    assert_equals_the_oracle(12345, ch, P.stream_lengths(plan), plan, f"12345 Hz x{ch} general kernel, rows in LDS")


# ---- 4. unaligned and pieced library PCM -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def short_episodes():
    return synth.make_library(3, 20.0, 6.0)


@pytest.mark.parametrize("rate,ch,key", [
    (384000, 2, ("general", "row", "global", "vec4", "n4")),
    (7350, 1, ("general", "contiguous", "global", "scalar", "n2048")),
    (2400, 2, ("general", "contiguous", "rows-in-lds", "vec4", "n32")),
    (11088, 2, ("mfma", "steps20", "rows-fit", "splits2", "waves<10")),
])
def test_library_pcm_unaligned_and_in_pieces(short_episodes, monkeypatch, rate, ch, key):
    """Three 20 s videos at `rate`: set_pcm_device from buffers 2 bytes past a 16-byte boundary (scalar staging, `odd`
    stereo loads) and set_pcm through a staging buffer of about three tiles (several pieces per window: resample_piece's
    rounding and the first_group / last_group fix-up on these layouts); hashes and timestamps are the oracle's."""
    from tests.test_gpu_library_rates import at_rate, device_copies, hashes_of, new_library, oracle_frame_hashes, oracle_hashes, windows
    plan = capi.resample_plan(rate)
    assert P.class_key(plan) == key
    n = len(short_episodes)
    pcms = [at_rate(e.pcm, rate, ch, k) for k, e in enumerate(short_episodes)]
    lens = [len(p) for p in pcms]
    ref = [oracle_hashes(oracle_frame_hashes(p, ch, rate)) for p in pcms]
    assert all(len(r[0]) > 20 and len(r[2]) > 5 for r in ref)
    bufs, ptrs = device_copies(pcms)
    assert all(p % 16 == 2 for p in ptrs)
    dev = new_library(n, rate)
    dev.set_pcm_device(ptrs, lens, channels=ch)
    del bufs
    dev.analyze(0, n)
    for v in range(n):
        assert hashes_of(dev.frame_hashes(v)) == ref[v], ("set_pcm_device", v)
    tile_values = plan["tile_outputs"] // plan["L"] * plan["M"] * ch
    (_, opening), _ = windows(lens[0], ch, rate)
    batch = int(3.3 * tile_values) + 1
    assert opening * ch > 4 * batch, "several pieces per window"
    monkeypatch.setenv("NEEDLE_HIP_MAX_BATCH_VALUES", str(batch))
    pieces = new_library(n, rate)
    pieces.set_pcm(pcms, lens, channels=ch)
    pieces.analyze(0, n)
    for v in range(n):
        assert hashes_of(pieces.frame_hashes(v)) == ref[v], ("set_pcm in pieces", v)


# ---- 5. a feeder whose lanes take four of the new plans ------------------------------------------------------------------------
MIXED = [(2, 384000, capi.SAMPLE_S16), (1, 7350, capi.SAMPLE_S16), (2, 11088, capi.SAMPLE_S16), (2, 48000, capi.SAMPLE_S16)]
MIXED_SECONDS = [20, 22, 21, 20]


def test_mixed_feeder_over_general_and_two_split_lanes():
    """Feeder.with_formats with lanes at 384000 / 2 (general, row, coefficients from global memory), 7350 / 1 (general,
    contiguous), 11088 / 2 (matrix cores, a tile cut in two) and 48000 / 2, fed in ragged chunks out of step: the items
    are Analyzer.run_pcm's of the same PCM at that rate, and the oracle's."""
    from tests.test_gpu_feeder_formats import feed_mixed
    from tests.test_gpu_feeder_ragged import content, one_shot
    streams, frames, want, raw = [], [], [], []
    for k in range(len(MIXED)):
        cfg = F.lane_config(k, MIXED, MIXED_SECONDS)
        c = content(cfg)
        streams.append(c["streams"][0])
        frames.append(c["frames"][0])
        want.append(one_shot(cfg, c)[0])
        raw.append(c["raw"][0][::F.STEP])
    assert frames == F.lane_frames(MIXED, MIXED_SECONDS)
    schedule = F.mixed_schedule(frames, MIXED)
    f = capi.Feeder.with_formats(MIXED, F.STEP)
    items = feed_mixed(f, MIXED, streams, schedule)
    for k in range(len(MIXED)):
        assert len(items[k]) > 50
        assert items[k].tolist() == want[k].tolist(), ("Analyzer.run_pcm", MIXED[k])
        assert items[k].tolist() == raw[k].tolist(), ("oracle", MIXED[k])
