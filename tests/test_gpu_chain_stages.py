"""GPU tests (-m gpu) of the certified fingerprint chain STAGE BY STAGE: what stft_chroma32_kernel, features_classify_cert_kernel,
the listed stft_chroma_kernel and fixup_items_kernel each wrote, read through needle_hip_fingerprint_stages_debug (the product's
own chain with device-to-device copies between its launches; capi.fingerprint_stages).  The other suites see the chain from
the outside only, and it hides its own mistakes: the first pass alone is right for all but one item in 80 000.

  (a) the first pass's chroma and energy rows at every launch geometry, against numpy's f64 chroma and the windowed frames'
      sums of squares;
  (b) the certification's decisions against the numpy statement of its rule on the first pass's own rows;
  (c) the recomputation and the fix-up with uncertain items on the edges of streams and chunks, bit for bit against the f64
      kernel alone.

Tolerances of (a): four times what the first pass stepped on the CPU (tests/cpu_emu, emu_stft_chroma_pair_f32's arithmetic)
shows against the same reference on the same frames; a missing bin or a lost energy partial is hundreds to thousands of
bounds away (tests/test_chain_stages_cpu.py).  On an MI355X the device turned out BIT-IDENTICAL to the emulation -- all 12
chroma values and all 4 energy partials of every row of (a), mono and stereo, every NEEDLE_STFT_PAIRS, and of the guided-ramp
launch's 15 232 rows -- so (a) asserts that equality, and the bounds beside it (which then hold by construction).

Measured (MI355X, profiles/NOTES.md), emulation = device, maxima over the rows of (a):
  row error / row's largest value : audio 3.33e-07 (bound 1.33e-06); noise of the guided ramp 1.87e-07; zoo 5.42e-06, not asserted
  row error / (u x pair energy)   : audio 0.681, zoo 0.609 mono and 0.736 stereo, guided ramp 0.067
  |energy sum / reference - 1|    : audio 6.62e-08, zoo 5.99e-08, guided ramp 6.22e-08 (the emulation test's bound is 1e-05)
(b): no decision of the device differed from the numpy rule outside the grey band at any step, tile size or K.
(c): no row or item differed.
"""
import functools

import numpy as np
import pytest

from needle_amd import capi
from oracle import oracle as O
from tests import chain_stages as S

pytestmark = pytest.mark.gpu

ENV = ("NEEDLE_HIP_STFT", "NEEDLE_HIP_CERT_K", "NEEDLE_STFT_PAIRS", "NEEDLE_HIP_ITEMS_PER_TILE", "NEEDLE_HIP_MAX_FRAMES_PER_CHUNK",
       "NEEDLE_HIP_SEPARATE_CLASSIFY", "NEEDLE_HIP_FALLBACK_GRID")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _env(monkeypatch, **values):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, v in values.items():
        if v is not None:
            monkeypatch.setenv(name, str(v))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _check_numbering(st, frames, step):
    """the hook's per-stream bases are plan_chunk's, and its counters agree with its lists"""
    ipt = st["items_per_tile"]
    assert st["streams"] == S.plan_streams(frames, step, ipt), (st["streams"], frames)
    assert st["chunks"] == (max(st["pairs"], 1) + st["chunk_pairs"] - 1) // st["chunk_pairs"]
    assert st["item_listed"].max(initial=0) <= 1 and st["chunk_listed"].max(initial=0) <= 1      # nothing listed twice
    assert st["items_listed"] == int(st["item_listed"].sum()) and st["chunks_listed"] == int(st["chunk_listed"].sum())


def _check_schedule(st):
    """every pair of the launch lies in exactly one workgroup of the schedule the first pass was given"""
    sched, pairs = st["schedule"], st["pairs"]
    seen = np.zeros(pairs, dtype=int)
    for b in range(8 * sched["blocks_per_xcd"]):
        f, l = S.block_range(sched, b, pairs)
        seen[f:l] += 1
    assert (seen == 1).all(), (sched, pairs)


# ---- (a) the first pass ----------------------------------------------------------------------------------------------------
# frames per stream; the key is the batch's pairs.  0 frames: fewer than 4096 samples.
BATCHES = {1: [0, 1], 2: [2, 0, 1], 7: [3, 1, 3, 2, 1], 8: [3, 1, 3, 2, 1, 2], 9: [1, 3, 2, 3, 0, 3, 1], 63: [41, 19, 1, 20, 21, 19],
           64: [23, 40, 3, 21, 1, 22, 2, 0, 3, 3, 3], 65: [21, 41, 23, 1, 40]}


def _batches():
    rng = np.random.default_rng(41)
    out = {}
    for pairs, frames in BATCHES.items():
        frames = [int(f) for f in rng.permutation(frames)]
        assert sum((f + 1) // 2 for f in frames) == pairs
        out[pairs] = frames
    every = [f for fr in out.values() for f in fr]
    assert set(every) == {0, 1, 2, 3, 19, 20, 21, 22, 23, 40, 41}
    bases = [s["pair_base"] for fr in out.values() for s in S.plan_streams(fr, 1) if s["frames"]]
    assert any(b % 2 for b in bases) and any(b and b % 2 == 0 for b in bases)                   # odd and even pair_base
    assert any(f % 2 for fr in out.values() for f in fr[:-1])                                   # a stream ends without frame B, mid-batch
    return out


@functools.lru_cache(maxsize=None)
def _first_pass_inputs(content, channels):
    """Per batch: the streams as fed, and per stream the f64 chroma, the pair energies and the emulated first pass; the bounds
    of the three measures: 4 x the emulation's maxima over all these frames."""
    rng = np.random.default_rng(1000 * channels + len(content))
    batches, emu_max = {}, np.zeros(3)
    for pairs, frames in _batches().items():
        streams = []
        for i, f in enumerate(frames):
            n = S.samples_for(f, extra=int(rng.integers(0, S.HOP)))
            mono = S.audio(200 + 16 * pairs + i, n) if content == "audio" else S.zoo_signal(S.ZOO[(i + pairs) % len(S.ZOO)], n, rng)
            if channels == 2:
                mono = np.clip(mono, -32760, 32760).astype(np.int16)
                fed = np.repeat(mono, 2) if not mono.any() else S.stereo_of(mono, rng)         # silence stays silence
                assert np.array_equal(S.mono_mix(fed), mono)
            else:
                fed = mono
            c64, e_pair = S.chroma64(mono), S.pair_energy(mono)
            c32, e4 = S.emu32(mono)
            if f:
                m1, m2 = S.row_errors(c32, c64, e_pair)
                emu_max = np.maximum(emu_max, [m1.max(), m2.max(), S.energy_errors(e4, e_pair).max()])
                if f % 2:                                                                       # an absent frame B adds exactly 0:
                    own = float(((mono[(f - 1) * S.HOP: (f - 1) * S.HOP + S.FRAME] * S.HALF_WINDOW) ** 2).sum())
                    assert e_pair[-1] == pytest.approx(own, rel=1e-12)                          # the last frame carries its own alone
            streams.append({"fed": fed, "mono": mono, "c64": c64, "e_pair": e_pair, "emu": (c32, e4)})
        batches[pairs] = streams
    assert np.isfinite(emu_max).all() and (emu_max > 0).all()
    return batches, 4.0 * emu_max, emu_max


@pytest.mark.parametrize("ppb", [None, 1, 3, 4, 16, 40])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("content", ["audio", "zoo"])
def test_first_pass_rows_and_energy_at_every_launch_geometry(content, channels, ppb, monkeypatch):
    """Ragged batches of 1, 2, 7, 8, 9, 63, 64 and 65 pairs (XCD parts empty, or of one pair) under NEEDLE_STFT_PAIRS unset, 1, 3,
    4, 16 and 40: no row of an existing frame keeps the hook's NaN sentinel, silent pairs are exact zeros, and every chroma
    row and energy sum is within four times the emulation's own error of the reference -- and, as measured, the emulation's
    bit for bit."""
    _env(monkeypatch, NEEDLE_STFT_PAIRS=ppb)
    batches, bound, emu_max = _first_pass_inputs(content, channels)
    worst, identical, rows = np.zeros(3), 0, 0
    for pairs, streams in batches.items():
        st = capi.fingerprint_stages([s["fed"] for s in streams], channels=channels, step=1)
        frames = [len(s["c64"]) for s in streams]
        assert st["pairs"] == pairs and st["frames"] == sum(frames)
        _check_numbering(st, frames, 1)
        _check_schedule(st)
        if ppb is not None:
            assert st["pairs_per_block"] == ppb
        assert not np.isnan(st["first_chroma"]).any() and not np.isnan(st["energy"]).any(), "a row no kernel wrote"
        assert not np.isnan(st["final_chroma"]).any()
        for s, m in zip(streams, st["streams"]):
            if not m["frames"]:
                continue
            c32 = st["first_chroma"][m["frame_base"]: m["frame_base"] + m["frames"]]
            e4 = st["energy"][m["frame_base"]: m["frame_base"] + m["frames"]]
            assert _same_bits(c32, c32.astype(np.float32).astype(np.float64))                   # f32 values, held as doubles
            m1, m2 = S.row_errors(c32, s["c64"], s["e_pair"])
            en = S.energy_errors(e4, s["e_pair"])
            silent = s["e_pair"] == 0
            assert (c32[silent] == 0).all() and (e4[silent] == 0).all()                         # exact zeros
            where = (pairs, m["frame_base"], m["frames"])
            if content == "audio":
                assert m1.max() <= bound[0], (where, int(np.argmax(m1)), m1.max(), bound[0])
            assert m2.max() <= bound[1], (where, int(np.argmax(m2)), m2.max(), bound[1])
            assert en.max() <= bound[2], (where, int(np.argmax(en)), en.max(), bound[2])
            if m["frames"] % 2:                                                                 # no frame B: the pair's energy is A's
                assert en[-1] <= bound[2]
            worst = np.maximum(worst, [m1.max() if content == "audio" else 0.0, m2.max(), en.max()])
            same = (_bits(c32) == _bits(s["emu"][0])).all(axis=1) & (e4.view(np.uint32) == s["emu"][1].view(np.uint32)).all(axis=1)
            assert same.all(), ("rows that are not the emulation's bit for bit", where, np.nonzero(~same)[0][:10])
            identical += int(same.sum())
            rows += m["frames"]
            got = st["items"][m["kept_base"]: m["kept_base"] + m["kept"]]
            assert got.tolist() == O.fingerprint(s["mono"]).tolist()
        if st["kept"] == 0:                                                                     # nothing to certify: the rows stay
            assert _same_bits(st["final_chroma"], st["first_chroma"]) and st["chunks_listed"] == 0
    print(f"first pass {content} ch{channels} ppb={ppb}: emulation max (row-max, energy-unit, energy) {emu_max}, device {worst}, "
          f"rows bit-identical to the emulation {identical}/{rows}")


def test_first_pass_on_the_smallest_launch_with_a_guided_ramp(monkeypatch):
    """The smallest launch stft32_schedule's guard (4 blocks >= 5 slots per XCD, 8 pairs per block) gives a ramp of half,
    quarter and eighth-size workgroups at the end of every XCD's part: noise as one long stream that ends without a frame B
    and a short second stream.  Every row against numpy's f64 chroma, and every size of workgroup in use on every XCD."""
    _env(monkeypatch, NEEDLE_STFT_PAIRS=8)
    cus = capi.fingerprint_stages([np.zeros(S.samples_for(1), np.int16)])["compute_units"]
    pairs = S.guided_pairs(cus, 8)
    frames = [2 * (pairs - 11) - 1, 21]
    if sum(frames) > 40000:
        pytest.skip(f"{cus} compute units put the guided ramp's smallest launch at {sum(frames)} frames")
    rng = np.random.default_rng(77)
    pcms = [rng.integers(-20000, 20000, S.samples_for(f, 5)).astype(np.int16) for f in frames]
    st = capi.fingerprint_stages(pcms, step=1)
    assert st["pairs"] == pairs and st["pairs_per_block"] == 8
    sched = st["schedule"]
    assert sched["sizes"] == [8, 4, 2, 1] and all(c > 0 for c in sched["counts"]), sched
    _check_numbering(st, frames, 1)
    _check_schedule(st)
    used = np.zeros((8, 4), dtype=int)
    for b in range(8 * sched["blocks_per_xcd"]):
        f, l = S.block_range(sched, b, pairs)
        used[b & 7, S.block_class(sched, b)] += l > f
    assert (used[:, 1:] > 0).all(), used                                                        # every XCD's ramp ran
    assert not np.isnan(st["first_chroma"]).any() and not np.isnan(st["energy"]).any()
    worst, emu_worst = np.zeros(3), np.zeros(3)
    for pcm, m in zip(pcms, st["streams"]):
        c64, e_pair = S.chroma64(pcm), S.pair_energy(pcm)
        oracle_chroma = O.fingerprint(pcm, debug=True)[1]
        assert np.abs(oracle_chroma - c64).max() <= 1e-11 * c64.max()                           # (the two references agree)
        emu_c, emu_e = S.emu32(pcm)
        rows = slice(m["frame_base"], m["frame_base"] + m["frames"])
        got = [*S.row_errors(st["first_chroma"][rows], c64, e_pair), S.energy_errors(st["energy"][rows], e_pair)]
        emu = [*S.row_errors(emu_c, c64, e_pair), S.energy_errors(emu_e, e_pair)]
        worst = np.maximum(worst, [g.max() for g in got])
        same = ((_bits(st["first_chroma"][rows]) == _bits(emu_c)).all(axis=1) &
                (st["energy"][rows].view(np.uint32) == emu_e.view(np.uint32)).all(axis=1))
        assert same.all(), ("rows that are not the emulation's bit for bit", np.nonzero(~same)[0][:10])
        emu_worst = np.maximum(emu_worst, [e.max() for e in emu])
        assert st["items"][m["kept_base"]: m["kept_base"] + m["kept"]].tolist() == O.fingerprint(pcm).tolist()
    print(f"guided ramp, {pairs} pairs on {cus} CUs: emulation max {emu_worst}, device {worst}, schedule {sched}")
    assert (worst <= 4 * emu_worst).all(), (worst, emu_worst)


# ---- (b) the certification -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def near():
    return S.near_snippets()


@pytest.mark.parametrize("tile", [1, 2, None])
@pytest.mark.parametrize("step", [1, 2, 3, 5])
def test_certification_decides_as_the_numpy_rule_on_its_own_rows(step, tile, near, monkeypatch):
    """At K = 64 and K = 8, steps 1, 2 (the SPLIT layout), 3 and 5, tiles of 1, 2 and the default number of items: which
    items features_classify_cert_kernel lists equals S.device_decisions on the hook's own first_chroma and energy, except
    within 1e-3 (relative) of the radius (at most 2 % of a case); the items it accepts are numpy's classification of those
    rows; the listed chunks are exactly the ones the listed items' frames span, each once; the counts are cert_stats'.
    Every case holds near-threshold snippets on its tile edges and noise under, over and AT the 0.01 norm cut (S.cert_case)."""
    ipt = S.tile_items(step, tile)
    pcms = S.cert_case(step, ipt, near)
    want = [O.fingerprint(p)[::step] for p in pcms]
    for k in (64, 8):
        _env(monkeypatch, NEEDLE_HIP_CERT_K=k, NEEDLE_HIP_ITEMS_PER_TILE=tile)
        capi.cert_stats(reset=True)
        st = capi.fingerprint_stages(pcms, step=step)
        stats = capi.cert_stats(reset=True)
        assert st["items_per_tile"] == ipt
        frames = [S.frames_of(len(p)) for p in pcms]
        _check_numbering(st, frames, step)
        assert [m["kept"] for m in st["streams"]][:6] == S.CERT_KEPT(ipt)
        listed = st["item_listed"].astype(bool)
        grey_total, compared = 0, 0
        for m, w in zip(st["streams"], want):
            rows = slice(m["frame_base"], m["frame_base"] + m["frames"])
            mine = slice(m["kept_base"], m["kept_base"] + m["kept"])
            refused, grey, bits = S.device_decisions(st["first_chroma"][rows], st["energy"][rows], float(k), step)
            assert len(refused) == m["kept"]
            grey_total += int(grey.sum())
            compared += int((~grey).sum())
            wrong = np.nonzero((listed[mine] != refused) & ~grey)[0]
            assert len(wrong) == 0, (k, m, wrong[:8], "listed by the device:", listed[mine][wrong[:8]])
            accepted = ~listed[mine]
            assert np.array_equal(st["first_items"][mine][accepted], bits[accepted]), (k, m)
            assert st["items"][mine].tolist() == w.tolist()                                     # and the chain's output is the oracle's
            assert np.array_equal(st["items"][mine][accepted], st["first_items"][mine][accepted])
        assert grey_total <= 0.02 * st["kept"], (grey_total, st["kept"])
        assert 0 < listed.sum() < st["kept"], "a case needs refused and accepted items"
        for i, m in enumerate(st["streams"][:6]):                                               # the planted items, on the tile edges
            if m["kept"]:
                assert listed[m["kept_base"] + m["kept"] - 1], (k, i)
        if k == 64:                                                                             # the row at the norm cut: its items
            m = st["streams"][-1]
            holds = np.arange(m["kept"]) * step <= S.NORM_CUT_ROW
            mine = listed[m["kept_base"]: m["kept_base"] + m["kept"]]
            assert mine[holds].all() and not mine.all(), (k, mine)
        chunks = S.listed_chunks(st["streams"], listed, step, st["chunk_pairs"], st["chunks"])
        assert np.array_equal(st["chunk_listed"].astype(bool), chunks)
        assert stats["items"] == st["kept"] and stats["items_recomputed"] == int(listed.sum()), stats
        assert stats["chunks"] == st["chunks"] and stats["chunks_recomputed"] == int(chunks.sum()), stats


# ---- (c) the recomputation and the fix-up -----------------------------------------------------------------------------------
EDGE_FRAMES = (45, 44, 20, 21, 22, 44)     # pairs 23, 22, 10, 11, 11, 22: pair_base 0, 23, 45, 55, 66, 77; 99 pairs, 50 chunks
SILENT_AT = 2                              # the variant with digital silence: 40 silent frames in front of stream 2


def _edge_plants(frames, step):
    """(stream, raw item) of every planted snippet: the last kept item of streams 0 (odd frames), 1 (even) and the last, the
    first item of stream 1 (behind an odd pair count: a chunk that straddles both), the only item of the 20-, 21- and
    22-frame streams"""
    last = lambda i: ((frames[i] - 20) // step) * step                                          # noqa: E731
    n = len(frames)
    return [(0, last(0)), (1, 0), (1, last(1)), (n - 4, 0), (n - 3, 0), (n - 2, 0), (n - 1, last(n - 1))]


@functools.lru_cache(maxsize=None)
def _edge_inputs(channels, step, silent):
    near = S.near_snippets()
    frames = list(EDGE_FRAMES)
    if silent:
        frames.insert(SILENT_AT, 40)
    rng = np.random.default_rng(7 + channels)
    monos = [S.audio(900 + i, S.samples_for(f, extra=int(rng.integers(0, S.HOP)))) for i, f in enumerate(frames)]
    if silent:
        monos[SILENT_AT][:] = 0
    for j, (i, k) in enumerate(_edge_plants(frames, step)):
        S.plant(monos[i], near[j % len(near)], k)
    fed = [m if channels == 1 else (np.repeat(m, 2) if not m.any() else S.stereo_of(m, rng)) for m in monos]
    return frames, monos, fed


@functools.lru_cache(maxsize=None)
def _f64_rows(channels, step, silent):
    """the f64 kernel alone over every stream (needle_hip_fingerprint_debug), checked against numpy at 1e-11 of the row's
    largest value; read with the environment of the caller (no variable set)"""
    frames, monos, fed = _edge_inputs(channels, step, silent)
    rows = []
    for mono, p in zip(monos, fed):
        chroma, _ = capi.fingerprint_debug(p, channels)
        ref = S.chroma64(mono)
        assert chroma.shape == ref.shape
        scale = np.maximum(ref.max(axis=1, keepdims=True), 1e-300)
        assert (np.abs(chroma - ref) <= 1e-11 * scale).all()
        rows.append(chroma)
    return np.concatenate(rows)


def _check_recomputation(st, f64, want, step, planted):
    listed, chunk_listed = st["item_listed"].astype(bool), st["chunk_listed"].astype(bool)
    row_chunk = S.chunk_of_rows(st["streams"], st["chunk_pairs"], st["frames"])
    inside = chunk_listed[row_chunk]
    assert np.array_equal(chunk_listed, S.listed_chunks(st["streams"], listed, step, st["chunk_pairs"], st["chunks"]))
    bad = np.nonzero((_bits(st["final_chroma"]) != _bits(f64)).any(axis=1) & inside)[0]
    assert len(bad) == 0, ("rows of listed chunks that are not the f64 kernel's", bad[:10], row_chunk[bad[:10]])
    bad = np.nonzero((_bits(st["final_chroma"]) != _bits(st["first_chroma"])).any(axis=1) & ~inside)[0]
    assert len(bad) == 0, ("rows outside every listed chunk that changed", bad[:10], row_chunk[bad[:10]])
    assert np.array_equal(st["items"][listed], want[listed])
    assert np.array_equal(st["items"][~listed], st["first_items"][~listed])
    assert np.array_equal(st["items"], want)
    for i, k in planted:
        m = st["streams"][i]
        assert listed[m["kept_base"] + k // step], ("a planted item was accepted", i, k)
    return listed, chunk_listed, row_chunk, inside


@pytest.mark.parametrize("beside", [False, True])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("channels", [1, 2])
def test_recomputation_and_fixup_on_the_edges_of_streams_and_chunks(channels, step, beside, monkeypatch):
    """Uncertain items planted on the edges: a chunk that straddles two streams, the last item of streams of odd and even
    frame counts, the only item of 20-, 21- and 22-frame streams, the batch's last, partial chunk; both forms of the listed
    kernel.  Rows inside listed chunks are the f64 kernel's bit for bit, every other row is the first pass's, listed items are
    the oracle's and the others the certification's.  The same with every item refused (K = 1e12) and none (K = 0), and
    with a silent stream in the batch."""
    _env(monkeypatch)
    frames, monos, fed = _edge_inputs(channels, step, False)
    f64 = _f64_rows(channels, step, False)
    want = np.concatenate([O.fingerprint(m)[::step] for m in monos])
    planted = _edge_plants(frames, step)
    st = capi.fingerprint_stages(fed, channels=channels, step=step, beside=beside)
    _check_numbering(st, frames, step)
    assert [m["pair_base"] for m in st["streams"]] == [0, 23, 45, 55, 66, 77] and st["pairs"] == 99 and st["chunks"] == 50
    listed, chunk_listed, row_chunk, inside = _check_recomputation(st, f64, want, step, planted)
    assert 0 < listed.sum() < st["kept"]
    # the straddling chunk holds rows of both streams, and both were recomputed (checked bit for bit above)
    s0, s1 = st["streams"][0], st["streams"][1]
    straddle = row_chunk[s1["frame_base"]]
    assert straddle == row_chunk[s0["frame_base"] + s0["frames"] - 1] and chunk_listed[straddle]
    assert chunk_listed[-1] and (row_chunk == st["chunks"] - 1).sum() == 2                      # the last chunk: one pair
    # teeth: a row the recomputation skipped could not hide -- the first pass's rows are not the f64 kernel's
    differs = (_bits(st["first_chroma"]) != _bits(f64)).any(axis=1)
    assert differs.mean() >= 0.99, differs.mean()
    assert (differs & inside).sum() >= 0.99 * inside.sum()

    _env(monkeypatch, NEEDLE_HIP_CERT_K=0)                                                      # nothing refused: nothing recomputed
    none = capi.fingerprint_stages(fed, channels=channels, step=step, beside=beside)
    assert none["items_listed"] == 0 and not none["chunk_listed"].any() and not none["item_listed"].any()
    assert _same_bits(none["final_chroma"], none["first_chroma"]) and _same_bits(none["first_chroma"], st["first_chroma"])
    assert np.array_equal(none["items"], none["first_items"])

    _env(monkeypatch, NEEDLE_HIP_CERT_K=1e12)                                                   # !(r < 0.25): every item with S > 0
    every = capi.fingerprint_stages(fed, channels=channels, step=step, beside=beside)
    assert every["item_listed"].all() and every["chunk_listed"].all()
    assert _same_bits(every["final_chroma"], f64)
    assert np.array_equal(every["items"], want)

    frames, monos, fed = _edge_inputs(channels, step, True)                                     # with digital silence
    f64 = _f64_rows(channels, step, True)
    want = np.concatenate([O.fingerprint(m)[::step] for m in monos])
    for k in (None, 1e12):
        _env(monkeypatch, NEEDLE_HIP_CERT_K=k)
        st = capi.fingerprint_stages(fed, channels=channels, step=step, beside=beside)
        _check_numbering(st, frames, step)
        listed, chunk_listed, row_chunk, inside = _check_recomputation(st, f64, want, step, _edge_plants(frames, step))
        m = st["streams"][SILENT_AT]
        assert m["kept"] > 0 and not listed[m["kept_base"]: m["kept_base"] + m["kept"]].any()   # silent items stay accepted
        rows = np.arange(m["frame_base"], m["frame_base"] + m["frames"])
        own = np.setdiff1d(row_chunk[rows], row_chunk[np.setdiff1d(np.arange(st["frames"]), rows)])
        assert len(own) >= 8 and not chunk_listed[own].any()                                   # ... and their chunks unlisted
        assert (st["first_chroma"][rows] == 0).all() and (st["final_chroma"][rows] == 0).all()
        if k is not None:                                                                       # everything else was refused
            others = np.ones(st["kept"], dtype=bool)
            others[m["kept_base"]: m["kept_base"] + m["kept"]] = False
            assert listed[others].all()


# ---- the hook itself -----------------------------------------------------------------------------------------------------------
def test_a_call_without_taps_launches_what_it_launched_before_the_hook_was_used(near, monkeypatch):
    from tests.test_gpu_feeder_formats import timed
    _env(monkeypatch)
    pcms = [S.audio(950 + i, S.samples_for(f)) for i, f in enumerate((45, 20, 64))] + [near[0]]
    before = timed(lambda: capi.fingerprint(pcms, step=2))
    assert all(before.get(k) == 1 for k in ("stft_chroma32", "features_cert", "stft_fallback", "fixup_items")), before
    items = capi.fingerprint(pcms, step=2)
    st = capi.fingerprint_stages(pcms, step=2, beside=True)
    after = timed(lambda: capi.fingerprint(pcms, step=2))
    assert after == before, (before, after)
    again = capi.fingerprint(pcms, step=2)
    assert [a.tolist() for a in again] == [a.tolist() for a in items]
    assert st["items"].tolist() == [x for a in items for x in a.tolist()]


def test_the_hook_refuses_what_it_cannot_show(monkeypatch):
    pcms = [S.audio(960 + i, S.samples_for(f)) for i, f in enumerate((30, 25))]
    _env(monkeypatch, NEEDLE_HIP_STFT="f64")
    with pytest.raises(capi.NeedleError):
        capi.fingerprint_stages(pcms)
    _env(monkeypatch, NEEDLE_HIP_MAX_FRAMES_PER_CHUNK=40)                                       # two chunks
    with pytest.raises(capi.NeedleError):
        capi.fingerprint_stages(pcms)
    _env(monkeypatch)
    st = capi.fingerprint_stages([np.zeros(100, np.int16)])                                     # not one frame: nothing runs
    assert st["frames"] == st["kept"] == st["chunks"] == 0 and len(st["items"]) == 0
    st = capi.fingerprint_stages(pcms)
    assert st["frames"] == 55 and st["kept"] == 17
