"""-m gpu: a feeder lane changes format in mid-stream and its fingerprint goes on (Feeder.switch_format).

A lane's stream is a list of PARTS; a part has a format, an optional channel mix, its samples, and says whether a switch
precedes it (a part without one continues the open segment).  The oracle of every case: per segment the front end alone
(capi.convert_mono or capi.rematrix_host, then capi.resample at any rate but 11025 Hz), the segments concatenated, then
capi.fingerprint over that mono PCM -- the feeder's items must equal it as arrays.  One case is checked against the CPU
oracle's resampler and fingerprinter as well (and numpy's conversion), so that the check does not rest on device code alone.
After every call of every case, ready's kept_items is needle_hip_feeder_num_ready_segments of lane_segments."""
from collections import namedtuple

import numpy as np
import pytest

from needle_amd import capi
from oracle import oracle as O
from tests import channel_mix as M
from tests import feeder_schedules as S
from tests.test_gpu_feeder import chunk_of, signal
from tests.test_gpu_feeder_formats import timed
from tests.test_gpu_library_rates import at_rate
from tests.test_gpu_matcher import by_source, one_shot
from tests.test_gpu_sample_formats import in_format, stream_of
from tests.test_sample_formats_cpu import to_s16

pytestmark = pytest.mark.gpu
STEP = 1
T = S.TARGET
S16, U8, S32, F32, F64 = capi.SAMPLE_S16, capi.SAMPLE_U8, capi.SAMPLE_S32, capi.SAMPLE_F32, capi.SAMPLE_F64
S16P, U8P, S32P, F32P, F64P = capi.SAMPLE_S16P, capi.SAMPLE_U8P, capi.SAMPLE_S32P, capi.SAMPLE_F32P, capi.SAMPLE_F64P
MASK_5_1 = 0x60F

Part = namedtuple("Part", "fmt mix stream frames switch")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


# ---- content and oracle -----------------------------------------------------------------------------------------------
def part(fmt, frames, seed, mix=None, switch=True, noise=False):
    """`frames` frames in the format: the tonal synth of the feeder tests (or seeded noise) brought to the rate and the
    channel count, then to the sample format with something below the s16 grid for the conversion to round."""
    ch, rate, sample_format = fmt
    n = -(-frames * T // rate) + 2
    mono = np.random.default_rng(seed).integers(-9000, 9000, n).astype(np.int16) if noise else signal(n, seed % 7)
    x = in_format(at_rate(mono, rate, ch, seed)[: frames * ch], sample_format, seed)
    assert len(x) == frames * ch
    return Part(fmt, mix, stream_of(x, ch, sample_format), frames, switch)


def seconds(fmt, s):
    return int(round(s * fmt[1]))


def segments_of(parts):
    """[(fmt, mix, [parts])]: the parts of each segment."""
    out = []
    for p in parts:
        if p.switch or not out:
            out.append((p.fmt, p.mix, [p]))
        else:
            assert out[-1][0] == p.fmt
            out[-1][2].append(p)
    return out


def joined(parts, fmt):
    """The parts of one segment as one stream."""
    if capi.sample_format_planar(fmt[2]):
        return [np.concatenate([p.stream[c] for p in parts]) for c in range(fmt[0])]
    return np.concatenate([p.stream for p in parts])


def oracle_mono(parts):
    """The lane's 11025 Hz mono signal: every segment landed and resampled as a whole stream of its own, concatenated."""
    out = []
    for fmt, mix, ps in segments_of(parts):
        if not sum(p.frames for p in ps):
            continue
        x = joined(ps, fmt)
        mono = (capi.rematrix_host([x], [fmt], [mix]) if mix is not None else capi.convert_mono([x], [fmt]))[0]
        assert len(mono) == sum(p.frames for p in ps)
        out.append(capi.resample([mono], 1, fmt[1])[0] if fmt[1] != T else mono)
    return np.concatenate(out) if out else np.zeros(0, np.int16)


def oracle_items(parts, step=STEP):
    return capi.fingerprint([oracle_mono(parts)], 1, step)[0]


def cpu_mono(parts):
    """The same without the device: numpy's conversion and fold-down, the CPU oracle's resampler."""
    out = []
    for fmt, mix, ps in segments_of(parts):
        ch, rate, sample_format = fmt
        if not sum(p.frames for p in ps):
            continue
        x = joined(ps, fmt)
        s16 = np.stack([to_s16(p, sample_format) for p in x], axis=1).reshape(-1) if capi.sample_format_planar(sample_format) else to_s16(x, sample_format)
        mono = M.fold_mono(s16, *mix.rows()) if mix is not None else M.plain_mono(s16, ch)
        out.append(O.resample(mono, 1, rate) if rate != T else mono)
    return np.concatenate(out)


# ---- the driver ----------------------------------------------------------------------------------------------------------
class Driven:
    """A feeder over lanes of parts.  Phase j: the lanes whose part j begins with a switch switch in ONE call, then part j
    of every lane is fed as `cut` says; lanes with fewer parts idle.  After every call: lane_segments is what was fed,
    ready is its host arithmetic, and the items so far extend the ones seen before."""

    def __init__(self, lanes, step=STEP, audit=False):
        self.lanes, self.step, self.n = lanes, step, len(lanes)
        self.f = capi.Feeder.with_formats([ps[0].fmt for ps in lanes], step)
        if audit:
            self.f.set_audit(True)
        mixed = [i for i, ps in enumerate(lanes) if ps[0].mix is not None]
        if mixed:
            self.f.set_lane_mix(mixed, [lanes[i][0].mix for i in mixed])
        self.want = [[(ps[0].fmt, 0)] for ps in lanes]
        self.finished = [False] * self.n
        self.seen = [np.zeros(0, dtype=np.uint32) for _ in range(self.n)]
        self.calls = 0

    def check(self):
        self.calls += 1
        for i in range(self.n):
            segs = self.f.lane_segments(i)
            assert segs == self.want[i], (self.calls, i, segs, self.want[i])
            assert self.f.lane_format(i) == segs[-1][0]
            want = (capi.num_ready_segments(segs, self.step, self.finished[i]), sum(n for _, n in segs), self.finished[i])
            assert self.f.ready(i) == want, (self.calls, i, self.f.ready(i), want)
            items = self.f.items(i)
            assert len(items) == want[0] and np.array_equal(items[: len(self.seen[i])], self.seen[i]), (self.calls, i)
            self.seen[i] = items

    def switch(self, lanes, formats, mixes=None):
        self.f.switch_format(lanes, formats, mixes)
        for i, fmt in zip(lanes, formats):
            self.want[i] = self.want[i] + [(fmt, 0)]
        self.check()

    def feed(self, chunks):
        """chunks: {lane: (part, first frame, frames)}"""
        row = [None] * self.n
        for i, (p, first, count) in chunks.items():
            row[i] = chunk_of(p.stream, p.fmt[0], p.fmt[2], first, count)
            self.want[i] = self.want[i][:-1] + [(self.want[i][-1][0], self.want[i][-1][1] + count)]
        self.f.feed(row)
        self.check()

    def phase(self, j, cut, seed=0):
        live = {i: ps[j] for i, ps in enumerate(self.lanes) if j < len(ps)}
        if cut == "empty":
            self.f.feed([None] * self.n)
            self.check()
        sw = [i for i, p in live.items() if j > 0 and p.switch]
        if sw:
            self.switch(sw, [live[i].fmt for i in sw], [live[i].mix for i in sw])
        if cut == "empty":
            self.f.feed([None] * self.n)
            self.check()
        if cut in ("whole", "empty"):
            cols = {i: [p.frames] for i, p in live.items()}
        elif cut == "1000":
            cols = {i: [min(1000, p.frames - a) for a in range(0, p.frames, 1000)] for i, p in live.items()}
        else:
            assert cut == "ragged"
            cols = {i: [r[0] for r in S.ragged_schedule([p.frames], p.fmt[1], seed + 31 * i + j)[0]] if p.frames else [] for i, p in live.items()}
        pos = {i: 0 for i in live}
        for r in range(max([len(c) for c in cols.values()] + [0])):
            chunks = {i: (live[i], pos[i], cols[i][r]) for i in live if r < len(cols[i]) and cols[i][r]}
            for i, (_, _, c) in chunks.items():
                pos[i] += c
            if chunks:
                self.feed(chunks)
        assert all(pos[i] == live[i].frames for i in live)

    def finish(self, lanes=None):
        self.f.finish(lanes)
        for i in (range(self.n) if lanes is None else lanes):
            self.finished[i] = True
        self.check()
        return self.seen


def drive(lanes, cut="whole", step=STEP, seed=0, audit=False):
    d = Driven(lanes, step, audit)
    for j in range(max(len(ps) for ps in lanes)):
        d.phase(j, cut, seed)
    d.finish()
    return d


def check_lanes(lanes, cut="whole", step=STEP, min_items=20):
    """min_items counts RAW items: a stream of 6 s has 27, one of 5.5 s has 23, and every `step`-th is kept."""
    d = drive(lanes, cut, step)
    for i, ps in enumerate(lanes):
        want = oracle_items(ps, step)
        assert len(want) >= -(-min_items // step), (i, len(want))
        assert np.array_equal(d.seen[i], want), (i, [(p.fmt, p.frames) for p in ps], cut)
    return d


# ---- 1. format sequences -----------------------------------------------------------------------------------------------
def mix_5_1():
    return capi.channel_mix_default(MASK_5_1)


def sequences():
    """The format sequences of the issue, 3-6 s per lane; u8 / s32 / f64, interleaved and planar, each beside a junction."""
    a = [(2, 48000, F32P), (2, 44100, S16)]
    b = [(2, 48000, S16), (1, T, S16), (2, 22050, S32)]
    c = [(1, T, U8), (2, 8000, F64P)]
    d = [(6, 48000, S16), (2, 48000, S16)]
    e = [(2, 44100, U8P), (3, 48000, S32P), (2, T, F64), (1, 22050, F32)]
    out = {}
    for name, fmts in dict(a=a, b=b, c=c, d=d, e=e).items():
        lens = {2: [3.0, 2.8], 3: [2.2, 1.6, 2.0], 4: [1.7, 1.3, 1.5, 1.4]}[len(fmts)]
        out[name] = [part(fmt, seconds(fmt, lens[k]) + 13 * k + 5, 10 * ord(name) + k,
                          mix=mix_5_1() if fmt[0] == 6 else None) for k, fmt in enumerate(fmts)]
    return out


_SEQ = {}


def seq(name):
    if not _SEQ:
        _SEQ.update(sequences())
    return _SEQ[name]


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_a_format_sequence_equals_the_fingerprint_of_the_concatenated_segments(name):
    d = check_lanes([seq(name)])
    print(name, [(p.fmt, p.frames) for p in seq(name)], "items", len(d.seen[0]), "calls", d.calls)


def test_one_sequence_against_the_cpu_oracle_and_under_the_f64_transform(monkeypatch):
    """Sequence e (four formats, three junctions; u8p, s32p, f64, f32) and d (a channel mix): numpy's conversion, the CPU
    oracle's resampler and its fingerprinter; then the same feeds under NEEDLE_HIP_STFT=f64."""
    for name in ("e", "d"):
        ps = seq(name)
        mono = cpu_mono(ps)
        assert np.array_equal(mono, oracle_mono(ps)), name
        want = O.fingerprint(mono)[::STEP]
        assert len(want) >= 20
        assert np.array_equal(drive([ps], "1000").seen[0], want), name
        assert np.array_equal(oracle_items(ps), want), name
    monkeypatch.setenv("NEEDLE_HIP_STFT", "f64")
    for name in ("e", "b"):
        assert np.array_equal(drive([seq(name)], "1000").seen[0], O.fingerprint(cpu_mono(seq(name)))[::STEP]), name


def test_several_lanes_switch_in_one_call_and_at_every_step():
    lanes = [seq(n) for n in "abcde"]
    for step in (2, 3):
        check_lanes(lanes, "1000", step)


# ---- 2. segment lengths --------------------------------------------------------------------------------------------------
def tile_inputs(rate):
    p = capi.resample_plan(rate)
    return -(-p["tile_outputs"] * p["M"] // p["L"]), p["tile_outputs"]


def test_the_tiles_are_the_ones_the_lengths_below_were_chosen_for():
    assert {r: tile_inputs(r)[1] for r in (44100, 48000, 22050, 8000)} == {44100: 1280, 48000: 2352, 22050: 1536, 8000: 7056}


@pytest.mark.parametrize("rate,fmt", [(44100, S16), (48000, F32), (22050, S32P), (8000, U8)])
def test_a_segment_of_zero_one_few_and_about_a_tile_s_frames(rate, fmt):
    """A middle segment at `rate` of 0 frames (two switches in a row), 1 frame, fewer than the filter's half length (no
    tile before the flush), and one tile's worth of input and that +- 1 -- each between 1.6 s at 48 kHz and 3.7 s at
    44.1 kHz or 11025 Hz, all in one feeder, the switches of every phase in one call."""
    half = S.tiling(rate)[2] if rate in S.TILE else 16
    n_tile = tile_inputs(rate)[0]
    lens = [0, 1, max(half - 3, 2), n_tile - 1, n_tile, n_tile + 1]
    lanes = []
    for k, n in enumerate(lens):
        first, last = (2, 48000, S16), ((1, T, S16) if k % 2 else (2, 44100, S16))
        lanes.append([part(first, seconds(first, 1.6) + k, 3 + k), part((1 + k % 2, rate, fmt), n, 50 + k, noise=True),
                      part(last, seconds(last, 3.7) + 3 * k, 20 + k)])
    check_lanes(lanes, "1000")
    # ... and with that segment first in the stream: the lane begins with it
    begun = []
    for k, ps in enumerate(lanes):
        last = ps[2].fmt
        begun.append([ps[1], part(last, seconds(last, 5.5) + 3 * k, 25 + k)])
    check_lanes(begun, "whole")


def frames_for_outputs(rate, lo, residue=None, mod=8):
    """The fewest frames at `rate` whose resampled length is >= lo (and == residue modulo `mod`)."""
    n = lo * rate // T
    while True:
        k = int(capi.lib().needle_hip_resample_out_len(n, rate))
        if k >= lo and (residue is None or k % mod == residue):
            return n
        n += 1


def test_the_junction_at_every_residue_of_the_sample_index_modulo_8():
    """48 kHz -> 11025 Hz s16 mono (the straight copy lands behind the flushed tail) -> 22.05 kHz (the first tile of a
    stream whose output 0 lies behind a carried tail), eight lanes: both junctions' 11025 Hz sample index takes every
    residue modulo 8."""
    lanes, residues = [], []
    for r in range(8):
        a = (2, 48000, S16)
        na = frames_for_outputs(48000, int(1.8 * T), r)
        nb = 3 * T // 2 + ((3 * r + 1) - r - 3 * T // 2) % 8                        # the second junction at residue (3 r + 1) % 8
        lanes.append([part(a, na, r), part((1, T, S16), nb, 30 + r), part((1, 22050, S16), seconds((1, 22050, 0), 2.2) + r, 40 + r)])
        first = int(capi.lib().needle_hip_resample_out_len(na, 48000))
        residues.append((first % 8, (first + nb) % 8))
    assert sorted(a for a, _ in residues) == list(range(8)) and sorted(b for _, b in residues) == list(range(8)), residues
    check_lanes(lanes, "whole")
    check_lanes(lanes, "1000")


# ---- 3. where in the stream the switch falls -------------------------------------------------------------------------------
def test_a_switch_inside_the_latency_beside_an_odd_frame_after_many_items_and_before_finish():
    a48, a11, b44, b22 = (2, 48000, S16), (1, T, S16), (2, 44100, S16), (1, 22050, F32)
    odd11 = S.FRAME + S.HOP * 20 + 700                                              # 21 whole frames: the 21st waits for its partner
    odd48 = frames_for_outputs(48000, S.FRAME + S.HOP * 22 + 5)                     # 23 whole frames after the flush
    lanes = [
        [part(a48, seconds(a48, 0.5), 1), part(b44, seconds(b44, 5.0), 2)],         # before the first item: 2 frames of 19
        [part(a11, 3000, 3), part(b22, seconds(b22, 5.0), 4)],                      # ... before the first frame
        [part(a11, odd11, 5), part(b44, seconds(b44, 2.8), 6)],                     # an odd trailing frame waits (no resampler before)
        [part(a48, odd48, 7), part(a11, 5 * T // 2, 8)],                            # ... and it is the flush that completes it
        [part(a48, seconds(a48, 4.5), 9), part(b22, seconds(b22, 1.2), 10)],        # carried rows after many items
        [part(a48, seconds(a48, 5.5), 11), part(b44, 0, 12)],                       # immediately before finish: the last segment is empty
        [part(a11, 11 * T // 2, 13), part(a48, 0, 14)],
    ]
    assert S.mirror(odd11, T, 1, STEP).frames == 20 and (odd11 - S.FRAME) // S.HOP + 1 == 21
    d = check_lanes(lanes, "1000")
    assert d.f.lane_segments(5)[-1] == (b44, 0) and d.f.lane_segments(6)[-1] == (a48, 0)
    check_lanes(lanes, "whole")


# ---- 4. neighbours ---------------------------------------------------------------------------------------------------------
def test_only_a_middle_lane_switches_and_its_neighbours_do_not_notice():
    fmts = [(1, T, S16), (2, 48000, S16), (2, 44100, S32), (1, 22050, U8), (6, 48000, F32P)]
    lanes = []
    for k, fmt in enumerate(fmts):
        first = part(fmt, seconds(fmt, 3.0) + 7 * k, 60 + k)
        if k == 1:
            lanes.append([first, part((2, 44100, S16), seconds((2, 44100, 0), 2.5), 70)])
        else:
            lanes.append([first, part(fmt, seconds(fmt, 2.5) + k, 80 + k, switch=False)])
    d = check_lanes(lanes, "1000")
    assert [len(d.f.lane_segments(i)) for i in range(5)] == [1, 2, 1, 1, 1]
    plain = drive([ps if k != 1 else ps[:1] for k, ps in enumerate(lanes)], "1000")  # nobody switches: lane 1 ends with its first part
    for k in (0, 2, 3, 4):
        assert np.array_equal(d.seen[k], plain.seen[k]), k
    # the flushed segment is the whole stream it would have been: what a lane that ends there emits is a prefix
    assert 0 < len(plain.seen[1]) < len(d.seen[1]) and np.array_equal(plain.seen[1], d.seen[1][: len(plain.seen[1])])


# ---- 5. cutting --------------------------------------------------------------------------------------------------------------
def test_the_items_do_not_depend_on_how_the_segments_were_cut_into_feeds():
    lanes = [seq("b"), seq("a"), seq("d"), seq("e")]
    want = [oracle_items(ps) for ps in lanes]
    for cut, seed in [("whole", 0), ("1000", 0), ("ragged", 1), ("ragged", 2), ("empty", 0)]:
        d = drive(lanes, cut, seed=seed)
        for i in range(len(lanes)):
            assert np.array_equal(d.seen[i], want[i]), (cut, seed, i)
        print(cut, seed, "calls", d.calls)


# ---- 6. a refused switch -------------------------------------------------------------------------------------------------------
def test_a_refused_switch_changes_nothing_and_the_stream_goes_on():
    fmts = [(2, 48000, S16), (1, T, S16), (2, 44100, F32)]
    lanes = [[part(fmt, seconds(fmt, 3.0), 90 + k), part(fmt, seconds(fmt, 2.5), 95 + k, switch=False)] for k, fmt in enumerate(fmts)]
    d = Driven(lanes)
    d.phase(0, "1000")
    state = d.f.state_bytes()
    for lanes_, formats, mixes in [([0, 1, 2], [(1, 8000, S16), (2, 22050, S16), (1, 44101, S16)], None),       # a bad rate in the last entry
                                   ([1, 0], [(1, 8000, S16), (2, 8000, S16)], [None, mix_5_1()]),               # a mix of six channels for two
                                   ([2, 0, 2], [(1, 8000, S16)] * 3, None), ([0, 3], [(1, 8000, S16)] * 2, None)]:
        with pytest.raises(capi.NeedleError) as e:
            d.f.switch_format(lanes_, formats, mixes)
        assert e.value.name == "InvalidArgument"
        d.check()                                                                   # segments, formats, ready, items: as they were
    assert d.f.state_bytes() == state and d.f.formats == fmts
    d.phase(1, "1000")
    d.finish([0, 1])
    with pytest.raises(capi.NeedleError) as e:                                      # a finished lane, named last
        d.f.switch_format([2, 0], [(1, 8000, S16), (1, 8000, S16)])
    assert e.value.name == "InvalidArgument"
    d.check()
    d.finish([2])
    for k, ps in enumerate(lanes):
        assert [len(s) for s in [d.f.lane_segments(k)]] == [1]
        assert np.array_equal(d.seen[k], oracle_items(ps)), k
    g = capi.Feeder(1, 2, 48000, S16, STEP)                                         # one format for all lanes: refused, and it goes on
    p0, p1 = lanes[0]
    g.feed([p0.stream])
    with pytest.raises(capi.NeedleError) as e:
        g.switch_format([0], [(2, 44100, S16)])
    assert e.value.name == "InvalidArgument" and g.lane_segments(0) == [(fmts[0], p0.frames)]
    g.feed([p1.stream])
    g.finish()
    assert np.array_equal(g.items(0), d.seen[0])


def test_set_audit_and_set_lane_mix_are_refused_after_a_switch_as_in_mid_stream():
    """A lane that was fed and then switched holds samples -- a tail and rows on the device -- although its open segment
    is empty: set_audit and set_lane_mix answer as they do in the middle of any stream, nothing changes, and the stream
    goes on to the oracle's items.  Lane 1 switches out of 11025 Hz (no flush), lane 0 out of 48 kHz."""
    a, b = (2, 48000, S16), (2, 44100, F32)
    lanes = [[part(a, seconds(a, 3.0), 41), part(b, seconds(b, 2.6), 42)],
             [part((1, T, S16), 3 * T, 43), part((6, 48000, S16), seconds(a, 2.6), 44, mix=mix_5_1())]]
    d = Driven(lanes)
    d.phase(0, "1000")
    for when in ("before the switch", "after it"):
        for call in (lambda: d.f.set_audit(True), lambda: d.f.set_audit(False),
                     lambda: d.f.set_lane_mix([0], [capi.ChannelMix.of([32768, 0], [0, 32768])]),
                     lambda: d.f.set_lane_mix([1], [None])):
            with pytest.raises(capi.NeedleError) as e:
                call()
            assert e.value.name == "InvalidArgument", when
            d.check()
        with pytest.raises(capi.NeedleError) as e:
            d.f.audit(0)                                                            # the audit is off, and stays off
        assert e.value.name == "InvalidArgument"
        if when == "before the switch":
            d.switch([0, 1], [lanes[0][1].fmt, lanes[1][1].fmt], [None, lanes[1][1].mix])
            assert [d.f.lane_segments(i)[-1][1] for i in range(2)] == [0, 0] and all(d.f.ready(i)[1] > 0 for i in range(2))
    for i, p in enumerate([lanes[0][1], lanes[1][1]]):
        d.feed({i: (p, 0, p.frames)})
    d.finish()
    for i, ps in enumerate(lanes):
        assert len(d.seen[i]) >= 20 and np.array_equal(d.seen[i], oracle_items(ps)), i
    d.f.reset()                                                                     # no lane holds samples: both are taken again
    d.f.set_lane_mix([1], [None])
    d.f.set_audit(True)
    assert d.f.audit(0)["items"] == 0


# ---- 7. the audit ----------------------------------------------------------------------------------------------------------------
def test_the_audit_runs_across_the_junctions():
    lanes = [seq("b"), seq("e"), seq("d")]
    d = drive(lanes, "1000", audit=True)
    for i, ps in enumerate(lanes):
        mono = oracle_mono(ps)
        g = capi.Feeder.with_formats([(1, T, S16)], STEP)
        g.set_audit(True)
        g.feed([mono])
        g.finish()
        assert np.array_equal(g.items(0), d.seen[i])
        a, b = d.f.audit(i), g.audit(0)
        assert set(a) >= {"items", "accepted", "accepted_mismatches", "mismatches", "max_error_over_s", "max_s"} and len(a) == 6
        assert a == b, (i, a, b)
        assert a["items"] == len(d.seen[i]) and a["accepted"] > 0 and a["mismatches"] == 0 and a["accepted_mismatches"] == 0


# ---- 8. into a matcher ---------------------------------------------------------------------------------------------------------------
def test_a_matcher_fed_from_the_feeder_across_a_switch_reports_the_one_shot_scan_s_runs():
    ps = seq("b")
    want_items = oracle_items(ps)
    other = oracle_items(seq("a"))
    sources, min_lens, t = [want_items, other, want_items[len(want_items) // 3:]], [12, 12, 12], 8
    want = one_shot(sources, min_lens, want_items, t)
    assert 0 in want and 2 in want and max(r[2] for r in want[0]) >= len(want_items) - 1   # the diagonal, across both junctions
    d = Driven([ps])
    m = capi.Matcher(sources, min_lens, 1, t)
    for j in range(len(ps)):
        d.phase(j, "1000")
        m.feed_from_feeder(d.f)
        assert m.ready(0)[1:] == (len(d.seen[0]), False)
    d.finish()
    m.feed_from_feeder(d.f)
    assert m.ready(0)[1:] == (len(want_items), True)
    assert by_source(m.runs(0)) == want


# ---- 9. launches and state -------------------------------------------------------------------------------------------------------------
def mono_bound(rate):
    """include/needle_hip.h's bound of state_bytes()[0] for a mono lane: 22 frames' rows and (24 x 1365 + 4096) samples of
    11025 Hz PCM -- 76 176 B -- and, at another rate, the inputs of one resampler tile plus its filter's length (and the 16
    samples its first one is rounded down by); with two channels at 48 kHz this is the header's 117 760 B."""
    if rate == T:
        return S.STATE_BOUND[(T, 1)]
    return S.STATE_BOUND[(T, 1)] + 2 * (tile_inputs(rate)[0] + 2 * S.tiling(rate)[2] + 16)


def test_what_a_switch_launches_and_what_a_switching_lane_carries():
    assert S.STATE_BOUND[(T, 1)] + 2 * (mono_bound(48000) - S.STATE_BOUND[(T, 1)]) == S.STATE_BOUND[(48000, 2)]
    a, quiet = (2, 48000, S16), (1, T, S16)
    one = part(a, seconds(a, 3.3), 1)                                               # (the flush completes a frame pair of it)
    calm = part(quiet, seconds(quiet, 3.3), 2)

    def fed(n):
        f = capi.Feeder.with_formats([a] * n + [quiet, a], STEP)
        f.feed([one.stream] * n + [calm.stream, None])
        assert f.ready(0)[0] > 0
        return f
    # lanes at 11025 Hz or without samples: nothing is launched
    f = fed(3)
    nothing = timed(lambda: f.switch_format([3, 4], [(2, 44100, S16), (1, 8000, U8)]))
    assert nothing == {}, nothing
    assert f.lane_segments(3) == [(quiet, calm.frames), ((2, 44100, S16), 0)] and f.lane_segments(4) == [(a, 0), ((1, 8000, U8), 0)]
    again = timed(lambda: f.switch_format([3, 4], [quiet, a]))                      # ... their open segments are empty now
    assert again == {}, again
    # resampling lanes: one flush round, the same launches for 2 and for 12 switching lanes
    counts = {}
    for k in (2, 12):
        f = fed(12)
        before = [f.ready(i)[0] for i in range(12)]
        counts[k] = timed(lambda: f.switch_format(list(range(k)), [(2, 44100, S16)] * k))
        assert all(f.ready(i)[0] >= before[i] for i in range(12))
        assert all(len(f.lane_segments(i)) == (2 if i < k else 1) for i in range(12))
    print("launches of a switch", counts)
    assert counts[2] == counts[12] and counts[2].get("resample") == 1 and counts[2].get("feeder_carry") == 1, counts
    assert counts[2].get("stft_chroma32") == 1, counts                              # the round goes on through the fingerprinter
    assert "ingest" not in counts[2] and "rematrix" not in counts[2], counts
    # state: 1-s chunks, a switch every four seconds between 48 kHz and 22.05 kHz / 11025 Hz
    cycle = [(2, 48000, S16), (1, 22050, S16), (2, 48000, F32), (1, T, S16)]
    chunks = {fmt: part(fmt, seconds(fmt, 1.0), 5 + k) for k, fmt in enumerate(cycle)}
    f = capi.Feeder.with_formats([cycle[0], cycle[1]], STEP)
    high = []
    for sec in range(32):
        if sec and sec % 4 == 0:
            f.switch_format([0, 1], [cycle[(sec // 4) % 4], cycle[(sec // 4 + 1) % 4]])
        now = [f.lane_format(0), f.lane_format(1)]
        f.feed([chunks[now[0]].stream, chunks[now[1]].stream])
        high.append(f.state_bytes()[0])
    print("state bytes over 32 s with seven switches", high[3], high[-1])
    assert 19 * 1365 * 2 < high[-1] <= mono_bound(48000), high
    assert high == sorted(high)
