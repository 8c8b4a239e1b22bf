"""-m gpu: the streaming fingerprinter's lanes fed out of step with each other.  One feed gives every lane a chunk of a
size of its own -- nothing, a few frames, a hop, a resampler tile, seconds -- by a schedule that meets the conditions
C1-C6 of tests/feeder_schedules.py, so that the lanes of one round differ in carry skew, in which of the feed's two
stream tables they are in, in the tiles they complete and in what they stage.  Every comparison is bit for bit: `ready`
against the host arithmetic after every round, the items so far a prefix that is never revised, and the finished items
against the one-shot path and against the oracle."""
import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O
from tests import feeder_schedules as S
from tests.test_gpu_crossmatcher import by_pair
from tests.test_gpu_crossmatcher_regions import one_shot as regions_one_shot
from tests.test_gpu_feeder import chunk_of, contested, counted, signal  # noqa: F401 (contested: a fixture)
from tests.test_gpu_library_rates import at_rate, hashes_of, oracle_hashes, results, windows
from tests.test_gpu_library_rates import oracle_frame_hashes as oracle_frame_hashes_at_rate
from tests.test_gpu_matcher import by_source
from tests.test_gpu_matcher import one_shot as matcher_one_shot
from tests.test_gpu_sample_formats import convert_spec, in_format, stream_of
from tests.test_gpu_scan_threshold import _dp_runs

pytestmark = pytest.mark.gpu
NS = O.NS
HASH_DURATION = {1: 0.15, 2: 0.3, 3: 0.4}                                       # seconds that make Analyzer.run_pcm keep every step-th item


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


# ---- the driver ---------------------------------------------------------------------------------------------------------
class Fed:
    """What feed_ragged knows of every lane: its stream, the frames fed, whether it is finished, the items seen."""

    def __init__(self, streams):
        n = len(streams)
        self.streams, self.pos, self.finished = list(streams), [0] * n, [False] * n
        self.seen = [np.zeros(0, dtype=np.uint32) for _ in range(n)]


def feed_ragged(f, streams, schedule, after_round=None):
    """One Feeder.feed per round with every lane's chunk in the same call, then `finish` for the lanes the schedule ends
    there.  After every round, for every lane: `ready` is the host arithmetic's count, and the items so far are the ones
    seen before plus a suffix.  after_round(r, state) may then look on (or reset a lane).  Returns the lanes' items."""
    rounds, finishes = schedule
    ch, rate, fmt, step = f.channels, f.sample_rate, f.sample_format, f.step
    st = Fed(streams)
    for r, (chunks, done) in enumerate(zip(rounds, finishes)):
        f.feed([chunk_of(st.streams[i], ch, fmt, st.pos[i], c) for i, c in enumerate(chunks)])
        st.pos = [p + c for p, c in zip(st.pos, chunks)]
        if done:
            f.finish(done)
            for i in done:
                st.finished[i] = True
        for i in range(f.lanes):
            want = (capi.feeder_num_ready(st.pos[i], rate, ch, step, st.finished[i]), st.pos[i], st.finished[i])
            assert f.ready(i) == want, (r, i)
            items = f.items(i)
            assert len(items) == want[0] and np.array_equal(items[: len(st.seen[i])], st.seen[i]), (r, i)
            st.seen[i] = items
        if after_round:
            after_round(r, st)
    assert all(st.finished)
    return st.seen


# ---- the configurations ---------------------------------------------------------------------------------------------------
_CONTENT, _RUNS = {}, {}


def content(cfg):
    """The lanes of a configuration, made once: streams in the format, cut to what the analyzer fingerprints of them
    (`whole`: before that cut, for Analyzer.run_pcm), their frames, and the oracle's raw items of the numpy-converted
    samples."""
    key = (cfg.rate, cfg.ch, cfg.fmt, cfg.seconds)
    if key not in _CONTENT:
        streams, whole, frames, raw = [], [], [], []
        for k, sec in enumerate(cfg.seconds):
            mono = signal(int(round(sec * S.TARGET)), 10 + k)
            x = mono if (cfg.rate, cfg.ch) == (S.TARGET, 1) else at_rate(mono, cfg.rate, cfg.ch, k)
            x = in_format(x, cfg.fmt, 50 + k)
            whole.append(stream_of(x, cfg.ch, cfg.fmt))
            n = S.whole_stream_window(len(x) // cfg.ch, cfg.rate)               # what the analyzer fingerprints of it
            x = x[: n * cfg.ch]
            s16 = convert_spec(x, cfg.ch, cfg.fmt % 5)
            raw.append(O.fingerprint(O.resample(s16, cfg.ch, cfg.rate)) if cfg.rate != S.TARGET else O.fingerprint(s16, channels=cfg.ch))
            streams.append(stream_of(x, cfg.ch, cfg.fmt))
            frames.append(n)
        assert frames == S.config_frames(cfg)
        _CONTENT[key] = dict(streams=streams, whole=whole, frames=frames, raw=raw)
    return _CONTENT[key]


def one_shot(cfg, c):
    """The lanes through the one-shot path: capi.fingerprint, or Analyzer.run_pcm with the window at the whole stream
    where a rate or a format is involved."""
    if (cfg.rate, cfg.fmt) == (S.TARGET, capi.SAMPLE_S16):
        return capi.fingerprint(c["streams"], cfg.ch, cfg.step)
    an = capi.Analyzer.from_files([f"lane{k}.wav" for k in range(len(c["whole"]))]).with_opening_search_percentage(1.0)
    fhs = an.run_pcm(c["whole"], channels=cfg.ch, sample_rate=cfg.rate, hash_duration=HASH_DURATION[cfg.step], sample_format=cfg.fmt)
    return [fh.opening_data()[0] for fh in fhs]


def run_config(name):
    """The configuration fed by its schedule, once: the conditions, the driver's checks, the one-shot and the oracle."""
    if name not in _RUNS:
        cfg = S.CONFIGS[name]
        c = content(cfg)
        schedule = S.ragged_schedule(c["frames"], cfg.rate, cfg.seed)
        S.check_conditions(schedule, cfg.rate, cfg.ch, cfg.step)
        f = capi.Feeder(len(c["frames"]), cfg.ch, cfg.rate, cfg.fmt, cfg.step)
        items = feed_ragged(f, c["streams"], schedule)
        want = one_shot(cfg, c)
        for k in range(f.lanes):
            assert items[k].tolist() == want[k].tolist(), (name, k)
            assert items[k].tolist() == c["raw"][k][:: cfg.step].tolist(), (name, k)
        assert sum(len(x) for x in items) > 50 and sum(len(x) > 0 for x in items) >= len(items) - 2   # (a: one lane is never fed, one holds 0.2 s)
        _RUNS[name] = dict(items=items, state=f.state_bytes(), schedule=schedule)
        print("state bytes", name, _RUNS[name]["state"], "rounds", len(schedule[0]))
    return _RUNS[name]


@pytest.mark.parametrize("name", sorted(S.CONFIGS))
def test_ragged_feeds_equal_the_one_shot_and_the_oracle(name):
    run_config(name)


@pytest.mark.parametrize("name", ["a1", "a2", "a3", "b", "c"])
def test_state_stays_within_the_documented_bound_when_lanes_are_out_of_step(name):
    """include/needle_hip.h's figure for the shape; and the high-water has seen a full tail (more than the 19 frames an
    item reaches back)."""
    cfg = S.CONFIGS[name]
    state = run_config(name)["state"][0]
    assert 19 * 1365 * 2 < state <= S.STATE_BOUND[(cfg.rate, cfg.ch)], state


# ---- the staging bound with several lanes -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a2", "c"])
def test_a_feed_of_several_lanes_is_cut_at_the_staging_bound(name, monkeypatch):
    """NEEDLE_HIP_MAX_BATCH_VALUES so small that the schedule's largest chunk alone is cut three times inside Feed and
    that some feed spends the bound before it reaches its last lane: the early pieces of such a feed give the later
    lanes nothing, the late pieces give the early lanes nothing."""
    cfg = S.CONFIGS[name]
    c, unbounded = content(cfg), run_config(name)
    schedule = unbounded["schedule"]
    bound, starved = S.staging_bound(schedule[0], cfg.ch)
    assert len(S.feed_pieces([max(max(r) for r in schedule[0])], bound, cfg.ch)) >= 4 and starved
    monkeypatch.setenv("NEEDLE_HIP_MAX_BATCH_VALUES", str(bound))
    f = capi.Feeder(len(c["frames"]), cfg.ch, cfg.rate, cfg.fmt, cfg.step)
    items = feed_ragged(f, c["streams"], schedule)
    staged = f.state_bytes()[1]
    monkeypatch.delenv("NEEDLE_HIP_MAX_BATCH_VALUES")
    assert staged <= 2 * bound, "no round staged more than the bound"
    for k in range(f.lanes):
        assert items[k].tolist() == unbounded["items"][k].tolist() == c["raw"][k][:: cfg.step].tolist(), k


# ---- reset in the middle ---------------------------------------------------------------------------------------------------
def test_a_lane_reset_while_its_neighbours_hold_state():
    """Configuration a at step 2: lane 1 is reset after a third of its stream, while lanes 0 and 4 hold tails and rows, and
    is then fed another stream by a schedule of its own."""
    cfg = S.CONFIGS["a2"]
    c = content(cfg)
    rounds, finishes = S.ragged_schedule(c["frames"], cfg.rate, cfg.seed)
    S.check_conditions((rounds, finishes), cfg.rate, cfg.ch, cfg.step)
    at = S.reset_round((rounds, finishes), cfg, lane=1, others=(0, 4))
    second = signal(8 * S.TARGET + 123, 30)
    rounds2, _ = S.ragged_schedule([len(second)], cfg.rate, 11)
    total = max(len(rounds), at + 1 + len(rounds2))
    rounds = [list(r) for r in rounds] + [[0] * len(c["frames"]) for _ in range(total - len(rounds))]
    finishes = [[i for i in done if i != 1] for done in finishes] + [[] for _ in range(total - len(finishes))]
    for r in range(at + 1, total):
        rounds[r][1] = rounds2[r - at - 1][0] if r - at - 1 < len(rounds2) else 0
    finishes[at + len(rounds2)].append(1)
    want = capi.fingerprint(c["streams"] + [second], 1, cfg.step)
    raw2 = (len(second) - S.FRAME) // S.HOP + 1 - S.LATENCY                    # 8 s: 62 frames, 43 raw items
    assert want[6].tolist() == O.fingerprint(second)[:: cfg.step].tolist() and len(want[6]) == -(-raw2 // cfg.step) > S.LATENCY
    f = capi.Feeder(6, 1, cfg.rate, cfg.fmt, cfg.step)
    first_part = []

    def reset(r, st):
        if r != at:
            return
        assert not st.finished[0] and not st.finished[4] and f.ready(0)[0] > 0 and f.ready(4)[0] > 0
        assert c["frames"][1] // 3 <= st.pos[1] < c["frames"][1] and not st.finished[1]
        first_part.append(st.seen[1])
        f.reset([1])
        assert f.ready(1) == (0, 0, False) and len(f.items(1)) == 0
        st.streams[1], st.pos[1], st.seen[1] = second, 0, np.zeros(0, dtype=np.uint32)
    items = feed_ragged(f, c["streams"], (rounds, finishes), after_round=reset)
    assert len(first_part[0]) > 3 and first_part[0].tolist() == want[1][: len(first_part[0])].tolist()
    assert items[1].tolist() == want[6].tolist()
    for k in (0, 2, 3, 4, 5):
        assert items[k].tolist() == want[k].tolist() == c["raw"][k][:: cfg.step].tolist(), k


# ---- contested content in several lanes -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contested_lanes(contested):
    lanes = list(contested) + [signal(S.CONTESTED_FRAMES[3], 41)]
    assert [len(x) for x in lanes] == S.CONTESTED_FRAMES
    return lanes, [O.fingerprint(x) for x in lanes]


def fed_contested(lanes, raw, step):
    schedule = S.ragged_schedule(S.CONTESTED_FRAMES, S.TARGET, S.CONTESTED_SEED)
    S.check_conditions(schedule, S.TARGET, 1, step)
    f = capi.Feeder(len(lanes), 1, S.TARGET, capi.SAMPLE_S16, step)
    items, many = counted(lambda: feed_ragged(f, lanes, schedule))
    for k in range(len(lanes)):
        assert items[k].tolist() == raw[k][::step].tolist(), k
    return many


@pytest.mark.parametrize("step", [2, 3])
def test_contested_content_in_lanes_out_of_step(contested_lanes, step):
    """The adversarial stream, two hostile episodes and an ordinary lane in one feeder: the content the first pass does
    not certify goes through tables whose prefixes differ.  The accept / recompute decisions are per item and do not
    depend on the neighbours: as many items classified and as many recomputed as in the four one-shot runs together."""
    lanes, raw = contested_lanes
    one = {"items": 0, "items_recomputed": 0}
    for k, pcm in enumerate(lanes):
        want, stats = counted(lambda: capi.fingerprint([pcm], 1, step)[0])
        assert want.tolist() == raw[k][::step].tolist()
        one = {key: one[key] + stats[key] for key in one}
    many = fed_contested(lanes, raw, step)
    print("cert stats", step, one, {key: many[key] for key in one})
    assert many["items"] == one["items"] == sum(len(x[::step]) for x in raw)
    assert many["items_recomputed"] == one["items_recomputed"] > 0


def test_contested_content_in_lanes_out_of_step_f64(contested_lanes, monkeypatch):
    lanes, raw = contested_lanes
    monkeypatch.setenv("NEEDLE_HIP_STFT", "f64")
    fed_contested(lanes, raw, 3)
    monkeypatch.delenv("NEEDLE_HIP_STFT")


# ---- down the chain, out of step, against the oracle ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def season():
    """Five episodes at 48 kHz stereo with their opening and ending windows cut as the analyzer cuts them, and the
    oracle's frame hashes and search results."""
    rate, ch = S.CHAIN_RATE, S.CHAIN_CH
    eps = synth.make_library(5, 90.0, 20.0, outro_s=15.0)
    pcms = [at_rate(e.pcm, rate, ch, k) for k, e in enumerate(eps)]
    ref = [oracle_frame_hashes_at_rate(p, ch, rate) for p in pcms]
    lanes, seeks = [], []
    for p in pcms:
        (o0, on), (e0, en, seek) = windows(len(p), ch, rate)
        lanes += [p[ch * o0: ch * (o0 + on)], p[ch * e0: ch * (e0 + en)]]
        seeks.append(seek)
    assert [len(x) // ch for x in lanes] == S.chain_frames()
    want = O.run_with_frame_hashes(O.Comparator(include_endings=True, min_opening_duration=10 * NS, min_ending_duration=10 * NS), ref)
    assert sum(w is not None and w.opening is not None for w in want) >= 3
    return dict(lanes=lanes, seeks=seeks, ref=ref, want=want)


def test_a_season_fed_out_of_step_into_a_crossmatcher_with_regions(season):
    rate, ch, step, videos = S.CHAIN_RATE, S.CHAIN_CH, S.CHAIN_STEP, 5
    t, min_len = 10, (30, 25)
    schedule = S.ragged_schedule(S.chain_frames(), rate, S.CHAIN_SEED)
    S.check_conditions(schedule, rate, ch, step)
    lanes, ref = season["lanes"], season["ref"]
    n = len(lanes)
    f = capi.Feeder(n, ch, rate, capi.SAMPLE_S16, step)
    cap = [max(capi.feeder_num_ready(len(lanes[k]) // ch, rate, ch, step, True) for k in range(r, n, 2)) for r in range(2)]
    m = capi.CrossMatcher.with_regions(videos, cap, min_len, t)

    def search(r, st):
        m.feed_from_feeder(f)
        assert [m.lane(k) for k in range(n)] == [(len(st.seen[k]), st.finished[k]) for k in range(n)], r
    items = feed_ragged(f, lanes, schedule, after_round=search)
    assert m.ready()[1]
    runs = m.runs()
    assert by_pair(runs) == regions_one_shot(items, videos, t, min_len)
    fhs = [f.frame_hashes(2 * v, 2 * v + 1, season["seeks"][v], hash_duration=HASH_DURATION[step]) for v in range(videos)]
    for v in range(videos):
        assert hashes_of(fhs[v]) == oracle_hashes(ref[v]), v
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(videos)], include_endings=True, min_opening_duration=10, min_ending_duration=10)
    assert results(cmp.results_from_runs(fhs, runs)) == results(season["want"])


def test_openings_fed_out_of_step_into_a_matcher(season):
    rate, ch, step = S.CHAIN_RATE, S.CHAIN_CH, S.CHAIN_STEP
    t, min_lens = 10, [30, 30]
    schedule = S.ragged_schedule(S.chain_frames(False), rate, S.OPENINGS_SEED)
    S.check_conditions(schedule, rate, ch, step)
    lanes, ref = season["lanes"][::2], season["ref"]
    sources = [np.array([h for h, _ in ref[v].opening], dtype=np.uint32) for v in (0, 3)]
    f = capi.Feeder(5, ch, rate, capi.SAMPLE_S16, step)
    m = capi.Matcher(sources, min_lens, 5, t)

    def search(r, st):
        m.feed_from_feeder(f)
        assert [m.ready(k)[1:] for k in range(5)] == [(len(st.seen[k]), st.finished[k]) for k in range(5)], r
    items = feed_ragged(f, lanes, schedule, after_round=search)
    found = 0
    for k in range(5):
        assert items[k].tolist() == [h for h, _ in ref[k].opening], k
        got = by_source(m.runs(k))
        assert got == matcher_one_shot(sources, min_lens, items[k], t), k
        dp = {q: sorted(_dp_runs(s, items[k], t, min_lens[q])) for q, s in enumerate(sources)}
        assert got == {q: v for q, v in dp.items() if v}, k
        found += len(got)
    assert found >= 6, "the shared intro is found in most lanes"
