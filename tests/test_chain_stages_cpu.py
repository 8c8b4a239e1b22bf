"""The tools of tests/test_gpu_chain_stages.py (tests/chain_stages.py) tested on their own, without a device: the numpy
statement of the acceptance rule against tools/f32_gate.py's, the error measures of the first pass against the two
mistakes they are there to catch, the chunk geometry against a brute-force enumeration."""
import importlib.util
import os

import numpy as np
import pytest

from needle_amd import synth
from tests import chain_stages as S
from tests import np_chromaprint as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def episode():
    """one episode, its f64 chroma and pair energies, and the first pass stepped on the CPU over it"""
    pcm = synth.make_episode(2, 40.0, 10.0).pcm[: 30 * 11025]
    c32, e4 = S.emu32(pcm)
    return {"pcm": pcm, "c64": S.chroma64(pcm), "e_pair": S.pair_energy(pcm), "c32": c32, "e4": e4}


def test_the_numpy_rule_agrees_with_the_gate_on_one_episode(episode):
    """tools/f32_gate.py refuses an item when its smallest |log v32 - t| is <= K S, S from each frame's own energy and no
    norm-cut clause.  The device's rule (S.device_rule) on the same rows -- the emulated first pass's -- with the gate's
    energies refuses the same items at every K of the gate's table, except where a row is at the norm cut (none on this
    episode) and inside the grey band; the counts are the gate's own."""
    spec = importlib.util.spec_from_file_location("f32_gate", os.path.join(ROOT, "tools", "f32_gate.py"))
    gate = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gate)
    pcm = synth.make_episode(5, 130.0, 10.0).pcm[: 120 * 11025]    # long enough for refusals at every K from 8 on
    table = gate.analyse(pcm, step=2)["ktable"]
    c32, e32 = gate.chroma_emu32(pcm)
    assert np.array_equal(c32, S.emu32(pcm)[0])
    own4 = np.zeros((len(c32), 4), dtype=np.float32)         # the gate's energies (each frame's own), as partials
    own4[:, 0] = e32 / S.ENERGY_SCALE
    vals, norm, scale = N.classifier_values(c32, e32)
    assert (np.abs(norm - 0.01) > 1e-4).all()
    margin = np.abs(vals[:, :, None] - S.THR[None]).min(axis=(1, 2))
    refusals = []
    for k in (4, 8, 16, 32, 64, 128, 256, 1024, 4096):
        refused, grey, _ = S.device_decisions(c32, own4, float(k), 2)
        want = (margin <= k * scale)[::2]
        if k in table:
            assert len(refused) == len(want) == table[k][1]
            assert int(want.sum()) == table[k][0]
        # log-distance r against relative distance r + r^2: the same decision outside a band of relative width ~r
        decided = ~grey & (np.abs(margin[::2] / np.maximum(k * scale[::2], 1e-300) - 1.0) > 1e-2)
        assert np.array_equal(refused[decided], want[decided]), k
        assert decided.mean() > 0.98
        refusals.append(int(want[decided].sum()))
    assert refusals[-1] > refusals[4] > 0, refusals          # ... and some of them were refusals, more as K grows


def _bin_powers(pcm):
    """|X_k|^2 of every frame over chromaprint's bins, [frames, 1298], and the bins' pitch classes"""
    k, note = N.note_table()
    idx = np.arange(S.frames_of(len(pcm)))[:, None] * S.HOP + np.arange(S.FRAME)[None, :]
    spec = np.fft.rfft(pcm[idx].astype(np.float64) * N.W64, axis=1)
    return (spec.real ** 2 + spec.imag ** 2)[:, k], note


def test_one_missing_bin_is_a_hundred_bounds_away(episode):
    """The chroma measures of (a) against the mistake they must catch: a pitch class that lacks one bin.  The bound of each
    measure is four times what the emulated first pass shows on the same frames.
    On noise (the guided-ramp case's content) EVERY one of the 1298 bins, left out of its class in every row as a kernel
    would leave it out, puts some row more than 100 bounds away in both measures (measured: 20 000), and a single row does
    so for more than 95 % of the bins.  On an episode, whose energy sits in a few partials, that holds for
    the strongest bin of each row's strongest class (measured: 80 000 bounds) and, with the bin missing from every row as a
    kernel would miss it, for about half of all bins; every bin is beyond the bound in some row (measured: 2.8 at least)."""
    rng = np.random.default_rng(7)
    noise = rng.integers(-20000, 20000, S.samples_for(24)).astype(np.int16)
    for pcm, c32, c64, e_pair in ((noise, S.emu32(noise)[0], S.chroma64(noise), S.pair_energy(noise)),
                                  (episode["pcm"], episode["c32"], episode["c64"], episode["e_pair"])):
        m1, m2 = S.row_errors(c32, c64, e_pair)
        bound1, bound2 = 4 * m1.max(), 4 * m2.max()
        assert 0 < bound1 < 8e-6                              # (the emulation test's own bound is 2e-6, times 4)
        power, note = _bin_powers(pcm)
        # the measures of a chroma that lacks bin b in row f, for every (f, b) at once: only that row's entry changes
        w1 = power / c64.max(axis=1)[:, None]
        w2 = power / (S.U * S.ENERGY_SCALE * e_pair)[:, None]
        wrong = c64.copy()                                    # (one of them through the function itself)
        wrong[3, note[500]] -= power[3, 500]
        g1, g2 = S.row_errors(wrong, c64, e_pair)
        assert np.isclose(g1[3], w1[3, 500], rtol=1e-6) and np.isclose(g2[3], w2[3, 500], rtol=1e-6)
        assert (np.delete(g1, 3) == 0).all()                  # ... and it names the row
        if pcm is noise:
            assert (w1.max(axis=0) > 100 * bound1).all() and (w2.max(axis=0) > 100 * bound2).all()
            assert (w1 > 100 * bound1).mean() > 0.95 and (w2 > 100 * bound2).mean() > 0.95   # (a single row: nearly always)
            continue
        top = np.argmax(c64, axis=1)
        strongest = np.array([power[f, note == top[f]].max() for f in range(len(c64))])
        assert (strongest / c64.max(axis=1) > 100 * bound1).all()
        assert (strongest / (S.U * S.ENERGY_SCALE * e_pair) > 100 * bound2).all()
        assert (w1.max(axis=0) > bound1).all() and (w2.max(axis=0) > bound2).all()
        assert (w1.max(axis=0) > 100 * bound1).mean() > 0.4 and (w2.max(axis=0) > 100 * bound2).mean() > 0.4


def test_one_lost_energy_partial_is_a_hundred_bounds_away(episode):
    e4, e_pair = episode["e4"], episode["e_pair"]
    err = S.energy_errors(e4, e_pair)
    bound = 4 * err.max()
    assert 0 < bound < 4e-5                                   # (the emulation test's own bound is 1e-5)
    for part in range(4):
        lost = e4.copy()
        lost[5, part] = 0.0
        bad = S.energy_errors(lost, e_pair)
        assert bad[5] > 100 * bound and (np.delete(bad, 5) <= bound).all(), (part, bad[5])
    nan = e4.copy()
    nan[9] = np.float32(np.nan)                               # the hook's sentinel: a row no kernel wrote
    assert S.energy_errors(nan, e_pair)[9] == np.inf
    c = episode["c32"].copy()
    c[9, 3] = np.nan
    assert S.row_errors(c, episode["c64"], e_pair)[0][9] == np.inf


def test_pair_energy_convention():
    rng = np.random.default_rng(4)
    pcm = rng.integers(-9000, 9000, S.samples_for(5, 17)).astype(np.int16)
    e = S.pair_energy(pcm)
    own = [float(((pcm[f * S.HOP: f * S.HOP + S.FRAME] * S.HALF_WINDOW) ** 2).sum()) for f in range(5)]
    assert np.allclose(e, [own[0] + own[1]] * 2 + [own[2] + own[3]] * 2 + [own[4]], rtol=1e-14)
    c32, e4 = S.emu32(pcm)                                    # the emulated kernel: the same convention, B absent adds 0
    assert (S.energy_errors(e4, e) < 1e-5).all()
    assert (S.pair_energy(np.zeros(S.samples_for(3), np.int16)) == 0).all()
    st = S.stereo_of(pcm, rng)
    assert np.array_equal(S.mono_mix(st), pcm) and (st[0::2] != st[1::2]).all()


@pytest.mark.parametrize("tile", [1, 2, None])
@pytest.mark.parametrize("step", [1, 2, 3, 5])
def test_the_certification_cases_hold_both_kinds_of_item_and_few_grey_ones(step, tile):
    """The inputs of the GPU test's part (b), chosen on the CPU: with the emulated first pass standing in for the device's
    (closer to it than numpy's f32 transform; on an MI355X the two are the same bits), every case at K = 64 and K = 8
    has refused and accepted items, the planted item of every stream is refused, the noise streams lie under, over and
    at the 0.01 norm cut -- at K = 64 the items that hold the row at the cut are refused by the norm clause and some of them
    by nothing else -- and at most 2 % of a case's items lie within 1e-3 of the radius."""
    ipt = S.tile_items(step, tile)
    pcms = S.cert_case(step, ipt, S.near_snippets())
    assert [S.plan_streams([S.frames_of(len(p))], step)[0]["kept"] for p in pcms[:6]] == S.CERT_KEPT(ipt)
    norms = [N.classifier_values(S.emu32(p)[0])[1] for p in pcms[6:]]
    assert norms[0].max() < 0.0098 and norms[1].min() > 0.0102                     # under and over the cut
    assert abs(norms[2][S.NORM_CUT_ROW] - 0.01) < 1e-6 and (norms[2] < 0.01).any() and (norms[2] > 0.01).any()
    for k in (64.0, 8.0):
        refused, grey = [], []
        for i, p in enumerate(pcms):
            r, g, _ = S.device_decisions(*S.emu32(p), k, step)
            if i < 6 and len(r):
                assert r[-1] and not g[-1], (k, i)
            refused.append(r)
            grey.append(g)
        if k == 64.0:                                                              # the norm clause alone refuses items here
            holds = np.arange(0, len(refused[-1]) * step, step) <= S.NORM_CUT_ROW
            assert refused[-1][holds].all() and not grey[-1][holds].any() and not refused[-1].all()
        refused, grey = np.concatenate(refused), np.concatenate(grey)
        assert 0 < refused.sum() < len(refused)
        assert grey.sum() <= 0.02 * len(grey), (k, int(grey.sum()), len(grey))


def test_the_norm_clause_alone_refuses_items_of_the_norm_cut_streams():
    """At K = 64 the streams with a row at the cut hold items that the rule refuses for a row at the cut and for nothing else
    (4, 9, 2 and 8 of the 12 items at steps 1, 2, 3 and 5: the chosen row's, and those of neighbours the noise left in the band)."""
    alone = {}
    for step in (1, 2, 3, 5):
        first = S.emu32(S.norm_cut_stream(19 + 12 * step, step))
        full, _ = S.device_rule(*first, 64.0, step)
        bare, _ = S.device_rule(*first, 64.0, step, norm_clause=False)
        assert not (bare & ~full).any()
        alone[step] = int((full & ~bare).sum())
    assert sum(v > 0 for v in alone.values()) >= 3, alone


# the stream shapes of part (c): frames per stream (tests/test_gpu_chain_stages.py EDGE_FRAMES), and ragged others
SHAPES = [(45, 44, 20, 21, 22, 44), (45, 44, 40, 20, 21, 22, 44), (20,), (21,), (22,), (1, 0, 23, 3, 41, 20, 19, 64)]


@pytest.mark.parametrize("frames", SHAPES)
@pytest.mark.parametrize("step", [1, 2, 3, 5])
@pytest.mark.parametrize("chunk_pairs", [1, 2, 4])
def test_chunk_geometry_against_brute_force(frames, step, chunk_pairs):
    """S.listed_chunks (the kernel's two-ended formula) against the enumeration of every frame of every item"""
    streams = S.plan_streams(frames, step)
    pairs = sum((f + 1) // 2 for f in frames)
    nchunks = (max(pairs, 1) + chunk_pairs - 1) // chunk_pairs
    kept = sum(s["kept"] for s in streams)
    row_chunk = S.chunk_of_rows(streams, chunk_pairs, sum(frames))
    assert row_chunk.max(initial=0) < nchunks
    for one in range(kept):                                   # every single item, then all of them
        listed = np.zeros(kept, dtype=bool)
        listed[one] = True
        want = np.zeros(nchunks, dtype=bool)
        s = [t for t in streams if t["kept_base"] <= one < t["kept_base"] + t["kept"]][0]
        x = (one - s["kept_base"]) * step
        for f in range(x, x + 20):
            if f < s["frames"]:
                want[row_chunk[s["frame_base"] + f]] = True
        assert x + 19 <= s["frames"] - 1                      # (an item never reaches past its stream; the clamp is inert)
        assert np.array_equal(S.listed_chunks(streams, listed, step, chunk_pairs, nchunks), want), one
    everything = S.listed_chunks(streams, np.ones(kept, dtype=bool), step, chunk_pairs, nchunks)
    touched = np.zeros(nchunks, dtype=bool)
    for s in streams:
        if s["kept"]:
            last = (s["kept"] - 1) * step + 19
            touched[row_chunk[s["frame_base"]: s["frame_base"] + last + 1]] = True
    assert np.array_equal(everything, touched)


def test_block_ranges_of_a_guided_schedule_cover_every_pair_once():
    """S.block_range (what the GPU test evaluates on the schedule the hook reports) on a schedule written out by hand"""
    sched = {"pairs_per_xcd": 96, "blocks_per_xcd": 10, "sizes": [24, 12, 6, 3], "counts": [2, 2, 2, 4]}
    total = 760                                               # the last XCD's part is short: its last workgroups are empty
    seen = np.zeros(total, dtype=int)
    for b in range(8 * sched["blocks_per_xcd"]):
        f, l = S.block_range(sched, b, total)
        seen[f:l] += 1
        assert S.block_class(sched, b) == [0, 0, 1, 1, 2, 2, 3, 3, 3, 3][b >> 3]
    assert (seen == 1).all()
    assert S.guided_pairs(256) == 7617
