"""-m gpu: the audit of the f32 first pass that travels with the stream (needle_hip_feeder_set_audit / _audit).

The yardstick is the one-shot audit, never the code under test: a capi.Library(n, opening_search_percentage=1.0) holding
the same streams at the same rate and format, with the hash duration that gives the feeder's step, analyze() and audit().
Every comparison is exact -- the four counts equal, max_error_over_s and max_s equal as doubles: they are integer counts
and maxima over the same per-item values, computed from rows that are the one-shot's bit for bit however the stream was
cut."""
import glob
import importlib.util
import json
import os
import re

import numpy as np
import pytest

from needle_amd import capi, synth
from tests import feeder_schedules as S
from tests.test_gpu_certified import _near_threshold_pairs
from tests.test_gpu_feeder import chunk_of, signal
from tests.test_gpu_library_rates import at_rate
from tests.test_gpu_sample_formats import in_format, stream_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASH_DURATION = {1: 0.15, 2: 0.3, 3: 0.4}        # seconds that make the library keep every step-th item
COUNTS = ("items", "accepted", "accepted_mismatches", "mismatches")
KEYS = COUNTS + ("max_error_over_s", "max_s")
ZERO = {k: 0 for k in KEYS}
# what a feed of s16 mono at 11025 Hz launches on the parent commit (feeder.hip, fingerprint.hip enqueue_certified)
PARENT_KERNELS = {"feeder_carry", "stft_chroma32", "features_cert", "stft_fallback", "fixup_items"}
AUDIT_KERNELS = {"audit_stft", "audit_items"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


@pytest.fixture(autouse=True)
def _product_mode(monkeypatch):
    for name in ("NEEDLE_HIP_STFT", "NEEDLE_HIP_CERT_K", "NEEDLE_HIP_MAX_BATCH_VALUES", "NEEDLE_HIP_MAX_FRAMES_PER_CHUNK"):
        monkeypatch.delenv(name, raising=False)


# ---- the yardstick and the driver -----------------------------------------------------------------------------------------
def library_audit(wholes, step, ch=1, rate=S.TARGET, fmt=capi.SAMPLE_S16):
    """needle_hip_library_audit over the whole streams as given (the library cuts its own whole-stream window)."""
    lib = capi.Library(len(wholes), opening_search_percentage=1.0, hash_duration=HASH_DURATION[step])
    if rate != S.TARGET:
        lib.set_sample_rate(rate)
    if fmt != capi.SAMPLE_S16:
        lib.set_sample_format(fmt)
    planar = capi.sample_format_planar(fmt)
    lib.set_pcm(wholes, [sum(len(p) for p in w) if planar else len(w) for w in wholes], channels=ch)
    lib.analyze()
    return lib.audit()


def frames_of(stream, ch, fmt):
    return len(stream[0]) if capi.sample_format_planar(fmt) else len(stream) // ch


def cut_to_window(whole, ch, rate, fmt):
    """What the library fingerprints of a stream with the window at 1.0: the feeder is fed exactly that."""
    n = S.whole_stream_window(frames_of(whole, ch, fmt), rate)
    return chunk_of(whole, ch, fmt, 0, n) if n else whole[:0], n


def uniform_schedule(lens, chunk):
    """Every lane `chunk` frames per round until its stream is spent; finished after the round that spends it."""
    n_rounds = max(1, max(-(-n // chunk) for n in lens))
    rounds = [[max(0, min(chunk, n - r * chunk)) for n in lens] for r in range(n_rounds)]
    finishes = [[i for i, n in enumerate(lens) if max(1, -(-n // chunk)) - 1 == r] for r in range(n_rounds)]
    return rounds, finishes


def feed_audited(f, streams, schedule, after_round=None, lanes=None):
    """Feeds by the schedule.  After every round -- a feed, and the finish behind it -- every lane's audit covers exactly
    the items `ready` reports and no count or maximum has fallen.  Returns the lanes' audits."""
    rounds, finishes = schedule
    ch, fmt = f.channels, f.sample_format
    lanes = list(range(f.lanes)) if lanes is None else lanes
    pos, prev = [0] * f.lanes, [dict(ZERO) for _ in range(f.lanes)]

    def look(r):
        for i in lanes:
            a = f.audit(i)
            assert a["items"] == f.ready(i)[0], (r, i, a)
            assert all(a[k] >= prev[i][k] for k in KEYS), (r, i, a, prev[i])
            prev[i] = a

    for r, (chunks, done) in enumerate(zip(rounds, finishes)):
        f.feed([chunk_of(streams[i], ch, fmt, pos[i], c) for i, c in enumerate(chunks)])
        pos = [p + c for p, c in zip(pos, chunks)]
        look(r)
        if done:
            f.finish(done)
            look(r)
        if after_round:
            after_round(r, pos, prev)
    return prev


def total_of(audits):
    out = {k: sum(a[k] for a in audits) for k in COUNTS}
    out.update({k: max(a[k] for a in audits) for k in ("max_error_over_s", "max_s")})
    return out


def same(a, b):
    return {k: a[k] for k in KEYS} == {k: b[k] for k in KEYS}


# ---- 1. any cutting equals the one-shot ---------------------------------------------------------------------------------
_EPISODES, _EPISODE_AUDITS = {}, {}


def episodes():
    if not _EPISODES:
        wholes = [synth.make_episode(30 + k, secs, 0.0).pcm for k, secs in enumerate((12.0, 35.0, 20.0, 8.0))]
        cut = [cut_to_window(w, 1, S.TARGET, capi.SAMPLE_S16) for w in wholes]
        _EPISODES.update(wholes=wholes, streams=[c[0] for c in cut], frames=[c[1] for c in cut])
        assert [(n - S.FRAME) // S.HOP + 1 for n in _EPISODES["frames"]] == [94, 280, 159, 62]
    return _EPISODES


def episode_audits(step):
    """The one-shot audits of the four episodes, once per step: four one-video libraries and the four in one."""
    if step not in _EPISODE_AUDITS:
        e = episodes()
        per_lane = [library_audit([w], step) for w in e["wholes"]]
        whole = library_audit(e["wholes"], step)
        assert same(whole, total_of(per_lane)) and whole["items"] > 0 and whole["mismatches"] == 0, (whole, per_lane)
        _EPISODE_AUDITS[step] = (per_lane, whole)
    return _EPISODE_AUDITS[step]


@pytest.mark.parametrize("cutting", ["one_chunk", "one_hop", "ragged"])
@pytest.mark.parametrize("step", [1, 2, 3])
def test_any_cutting_equals_the_one_shot_audit(step, cutting):
    e = episodes()
    per_lane, whole = episode_audits(step)
    schedule = {"one_chunk": lambda: uniform_schedule(e["frames"], max(e["frames"])),
                "one_hop": lambda: uniform_schedule(e["frames"], S.HOP),
                "ragged": lambda: S.ragged_schedule(e["frames"], S.TARGET, 7 + step)}[cutting]()
    f = capi.Feeder(4, 1, S.TARGET, capi.SAMPLE_S16, step)
    f.set_audit(True)
    totals = []

    def total_grows(r, pos, prev):
        t = f.audit()
        assert same(t, total_of(prev)), (r, t, prev)
        totals.append(t)

    got = feed_audited(f, e["streams"], schedule, after_round=total_grows)
    print("feeder audit, step", step, cutting, ":", got, "one-shot:", per_lane)
    for i in range(4):
        assert same(got[i], per_lane[i]), (i, got[i], per_lane[i])
    assert same(f.audit(), whole), (f.audit(), whole)
    assert all(all(b[k] >= a[k] for k in KEYS) for a, b in zip(totals, totals[1:]))


# ---- 2. the audit disturbs nothing -----------------------------------------------------------------------------------------
def test_the_audit_disturbs_neither_the_items_nor_the_cert_stats():
    e = episodes()
    schedule = S.ragged_schedule(e["frames"], S.TARGET, 9)
    want = capi.fingerprint(e["streams"], 1, 2)

    def run(on):
        f = capi.Feeder(4, 1, S.TARGET, capi.SAMPLE_S16, 2)
        if on:
            f.set_audit(True)
        capi.cert_stats(reset=True)
        rounds, finishes = schedule
        pos = [0] * 4
        for chunks, done in zip(rounds, finishes):
            f.feed([chunk_of(e["streams"][i], 1, capi.SAMPLE_S16, pos[i], c) for i, c in enumerate(chunks)])
            pos = [p + c for p, c in zip(pos, chunks)]
            if done:
                f.finish(done)
        items = [f.items(i).tolist() for i in range(4)]
        return items, capi.cert_stats(reset=True)

    off_items, off_stats = run(False)
    on_items, on_stats = run(True)
    assert on_items == off_items == [w.tolist() for w in want]
    assert on_stats == off_stats and off_stats["items"] == sum(len(w) for w in want), (on_stats, off_stats)


# ---- 3. the audit is not vacuous -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def adversarial():
    pairs = _near_threshold_pairs(40, seed=17)      # the call tests/test_gpu_certified.py's fixture makes
    assert len(pairs) >= 30
    return [p for lo, hi, *_ in pairs for p in (lo, hi)]


def _feeder_total(pcms, chunk):
    f = capi.Feeder(len(pcms), 1, S.TARGET, capi.SAMPLE_S16, 1)
    f.set_audit(True)
    feed_audited(f, pcms, uniform_schedule([len(p) for p in pcms], chunk), lanes=[0, len(pcms) // 2, len(pcms) - 1])
    return f.audit()


def test_the_audit_finds_what_the_radius_prevents(adversarial, monkeypatch):
    """One lane per near-threshold snippet (60-80 lanes), chunks of 5000 samples.  With the product's K every item was
    refused by the first pass; with NEEDLE_HIP_CERT_K=0 the one-shot audit reports accepted items whose f32 bits are
    wrong -- the precondition on the reference -- and the feeder's audit reports exactly the same."""
    n = len(adversarial)
    assert 60 <= n <= 80
    a = _feeder_total(adversarial, 5000)
    assert a["items"] == n and a["accepted"] == 0 and a["mismatches"] == 0 and a["accepted_mismatches"] == 0, a
    assert same(a, library_audit(adversarial, 1))
    monkeypatch.setenv("NEEDLE_HIP_CERT_K", "0")
    ref = library_audit(adversarial, 1)
    assert ref["accepted_mismatches"] >= 1, ref
    b = _feeder_total(adversarial, 5000)
    print("K = 0: feeder", b, "library", ref)
    assert same(b, ref), (b, ref)
    assert b["items"] == n and b["accepted"] == n and b["mismatches"] >= 1


# ---- 4. the golden adversarial corpus --------------------------------------------------------------------------------------
def test_golden_adversarial_corpus_lane_by_lane():
    spec = importlib.util.spec_from_file_location("fuzz_cert_adversarial", os.path.join(ROOT, "tools", "fuzz_cert_adversarial.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    corpus = json.load(open(os.path.join(ROOT, "tests", "golden", "cert_adversarial.json")))
    thetas = [corpus["before_pair_energy"]["theta"]] + [v["theta"] for v in corpus["after_pair_energy"]["families"].values()]
    thetas += [v["theta"] for v in corpus.get("round6", {}).get("families", {}).values()]
    wholes = [fz.synth(np.array(th)) for th in thetas]
    assert len(wholes) >= 1 + len(fz.FAMILIES)
    cut = [cut_to_window(w, 1, S.TARGET, capi.SAMPLE_S16) for w in wholes]
    f = capi.Feeder(len(wholes), 1, S.TARGET, capi.SAMPLE_S16, 1)
    f.set_audit(True)
    got = feed_audited(f, [c[0] for c in cut], S.ragged_schedule([c[1] for c in cut], S.TARGET, 4))
    for i, w in enumerate(wholes):
        want = library_audit([w], 1)
        assert same(got[i], want), (i, got[i], want)
        kept = int(capi.lib().needle_hip_fingerprint_num_kept(cut[i][1], 1))     # (the window's rounding may cost the last sample)
        assert got[i]["items"] == kept >= fz.ITEMS - 1 and got[i]["accepted_mismatches"] == 0 and got[i]["mismatches"] == 0, (i, got[i])
        assert got[i]["max_error_over_s"] < 8.0, (i, got[i])
    total = f.audit()
    assert same(total, library_audit(wholes, 1)) and total["accepted"] > 0, total
    # ... and to the last sample, against the one-shot audit the corpus was searched with
    f = capi.Feeder(len(wholes), 1, S.TARGET, capi.SAMPLE_S16, 1)
    f.set_audit(True)
    feed_audited(f, wholes, S.ragged_schedule([len(w) for w in wholes], S.TARGET, 5))
    full, want = f.audit(), fz.Auditor(len(wholes)).audit(wholes)
    assert same(full, want) and full["items"] == len(wholes) * fz.ITEMS, (full, want)
    assert full["accepted_mismatches"] == 0 and full["mismatches"] == 0 and full["max_error_over_s"] < 8.0, full


# ---- 5. other doors --------------------------------------------------------------------------------------------------------
DOORS = {"f32p_stereo_48k": (48000, 2, capi.SAMPLE_F32P, 2), "s16_six_channels_48k": (48000, 6, capi.SAMPLE_S16, 1)}
_DOORS = {}


def door(name):
    if name not in _DOORS:
        rate, ch, fmt, lanes = DOORS[name]
        wholes = []
        for k in range(lanes):
            x = in_format(at_rate(signal(10 * S.TARGET, 20 + k), rate, ch, k), fmt, 60 + k)
            wholes.append(stream_of(x, ch, fmt))
        cut = [cut_to_window(w, ch, rate, fmt) for w in wholes]
        per_lane = [library_audit([w], 2, ch, rate, fmt) for w in wholes]
        whole = library_audit(wholes, 2, ch, rate, fmt)
        assert whole["items"] >= 25 * lanes and whole["mismatches"] == 0 and whole["accepted_mismatches"] == 0, whole
        _DOORS[name] = dict(streams=[c[0] for c in cut], frames=[c[1] for c in cut], per_lane=per_lane, whole=whole)
    return _DOORS[name]


@pytest.mark.parametrize("cutting", ["one_second", "ragged"])
@pytest.mark.parametrize("name", sorted(DOORS))
def test_other_rates_formats_and_channel_counts(name, cutting):
    rate, ch, fmt, lanes = DOORS[name]
    d = door(name)
    schedule = uniform_schedule(d["frames"], rate) if cutting == "one_second" else S.ragged_schedule(d["frames"], rate, 3)
    f = capi.Feeder(lanes, ch, rate, fmt, 2)
    f.set_audit(True)
    got = feed_audited(f, d["streams"], schedule)
    for i in range(lanes):
        assert same(got[i], d["per_lane"][i]), (i, got[i], d["per_lane"][i])
    assert same(f.audit(), d["whole"]), (f.audit(), d["whole"])


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------
def test_a_stream_without_an_item_and_a_stream_with_an_odd_last_frame():
    short = signal(S.FRAME + 9 * S.HOP + 300, 41)                       # 10 frames: inside the latency
    odd = signal(S.FRAME + 40 * S.HOP + 700, 42)                  # 41 frames: the last one has no partner
    streams = [cut_to_window(x, 1, S.TARGET, capi.SAMPLE_S16)[0] for x in (short, odd)]
    assert [(len(x) - S.FRAME) // S.HOP + 1 for x in streams] == [10, 41]
    for step in (1, 2):
        f = capi.Feeder(2, 1, S.TARGET, capi.SAMPLE_S16, step)
        f.set_audit(True)
        got = feed_audited(f, streams, uniform_schedule([len(x) for x in streams], 3 * S.HOP + 11))
        assert got[0] == ZERO, got[0]
        want = library_audit([odd], step)
        assert want["items"] == -(-(41 - S.LATENCY) // step)
        assert same(got[1], want) and same(f.audit(), want), (got[1], want)


def test_a_reset_lane_audits_its_second_stream_and_leaves_its_neighbours_alone():
    first = [signal(9 * S.TARGET + 17 * k, 50 + k) for k in range(3)]
    second = signal(7 * S.TARGET + 5, 59)
    cut = lambda x: cut_to_window(x, 1, S.TARGET, capi.SAMPLE_S16)[0]                  # noqa: E731
    streams = [cut(x) for x in first]
    chunk = 9000                                                                   # five rounds: 30 whole frames, 6 kept items
    f = capi.Feeder(3, 1, S.TARGET, capi.SAMPLE_S16, 2)
    f.set_audit(True)
    rounds, finishes = uniform_schedule([len(x) for x in streams], chunk)
    pos = [0, 0, 0]
    for r in range(5):                                                             # five rounds of all three lanes
        f.feed([chunk_of(streams[i], 1, capi.SAMPLE_S16, pos[i], rounds[r][i]) for i in range(3)])
        pos = [p + c for p, c in zip(pos, rounds[r])]
    before = [f.audit(i) for i in range(3)]
    assert all(a["items"] == f.ready(i)[0] > 0 for i, a in enumerate(before))
    f.reset([1])
    assert f.audit(1) == ZERO and f.audit(0) == before[0] and f.audit(2) == before[2]
    streams[1], pos[1] = cut(second), 0
    lens = [len(x) for x in streams]
    while any(p < n for p, n in zip(pos, lens)):
        chunks = [min(chunk, n - p) for p, n in zip(pos, lens)]
        f.feed([chunk_of(streams[i], 1, capi.SAMPLE_S16, pos[i], chunks[i]) for i in range(3)])
        pos = [p + c for p, c in zip(pos, chunks)]
        assert all(f.audit(i)["items"] == f.ready(i)[0] for i in range(3))
    f.finish()
    for i, whole in enumerate((first[0], second, first[2])):
        want = library_audit([whole], 2)
        assert same(f.audit(i), want) and want["items"] > 10, (i, f.audit(i), want)
    assert same(f.audit(), library_audit([first[0], second, first[2]], 2))


# ---- 7. refusals and launches ------------------------------------------------------------------------------------------------
def _invalid(call):
    with pytest.raises(capi.NeedleError) as e:
        call()
    assert e.value.name == "InvalidArgument", e.value
    return str(e.value)


def test_refusals(monkeypatch):
    whole = signal(6 * S.TARGET, 70)
    x = cut_to_window(whole, 1, S.TARGET, capi.SAMPLE_S16)[0]
    want = capi.fingerprint([x], 1, 2)[0].tolist()
    f = capi.Feeder(2, 1, S.TARGET, capi.SAMPLE_S16, 2)
    _invalid(lambda: f.audit(0))                                                    # the audit is off
    _invalid(lambda: f.audit())
    f.feed([None, x[:30000]])
    _invalid(lambda: f.set_audit(True))                                             # a lane holds samples: nothing changed
    _invalid(lambda: f.audit(1))
    f.feed([None, x[30000:]])
    f.finish([1])
    assert f.items(1).tolist() == want
    f.reset()
    f.set_audit(True)                                                               # every lane reset: allowed again
    _invalid(lambda: f.audit(2))                                                    # a lane out of range
    f.feed([x[:30000], None])
    _invalid(lambda: f.set_audit(False))
    f.feed([x[30000:], None])
    f.finish([0])
    assert f.items(0).tolist() == want and f.audit(0)["items"] == len(want) and f.audit(1) == ZERO
    # NEEDLE_HIP_STFT=f64: there is no first pass to audit
    monkeypatch.setenv("NEEDLE_HIP_STFT", "f64")
    g = capi.Feeder(1, 1, S.TARGET, capi.SAMPLE_S16, 2)
    assert "f64" in _invalid(lambda: g.set_audit(True))
    g.feed([x[:30000]])                                                             # unaudited, f64 mode feeds as ever
    monkeypatch.delenv("NEEDLE_HIP_STFT")
    h = capi.Feeder(1, 1, S.TARGET, capi.SAMPLE_S16, 2)
    h.set_audit(True)
    h.feed([x[:30000]])
    seen = h.ready(0)
    monkeypatch.setenv("NEEDLE_HIP_STFT", "f64")
    assert "f64" in _invalid(lambda: h.feed([x[30000:]]))                           # refused before any device work ...
    assert h.ready(0) == seen
    monkeypatch.delenv("NEEDLE_HIP_STFT")
    h.feed([x[30000:]])                                                             # ... so the stream goes on where it was
    h.finish()
    assert h.items(0).tolist() == want and same(h.audit(0), library_audit([whole], 2))


def _timer_names():
    """Every name a KernelTimer is made with, read from the sources: the kernels kernel timing can show."""
    names = set()
    for path in glob.glob(os.path.join(ROOT, "needle_amd", "csrc", "*.hip")):
        names |= set(re.findall(r'KernelTimer\w*\s*(?:\w+)?\(\s*"(\w+)"', open(path).read()))
    assert PARENT_KERNELS | AUDIT_KERNELS <= names and len(names) > 25
    return names


def _kernels_shown(audit, rate, ch, fmt, stream, frames):
    f = capi.Feeder(2, ch, rate, fmt, 2)
    if audit:
        f.set_audit(True)
    names = _timer_names()
    capi.set_kernel_timing("all,sum")
    try:
        pos = 0
        while pos < frames:
            c = min(rate, frames - pos)
            f.feed([chunk_of(stream, ch, fmt, pos, c), None])
            pos += c
        f.finish()
        f.ready(0)
        return {k for k in names if capi.last_kernel_ms(k) >= 0}
    finally:
        capi.set_kernel_timing(None)


def test_an_unaudited_feed_launches_what_it_did_and_an_audited_one_two_kernels_more():
    x = signal(5 * S.TARGET, 71)
    off = _kernels_shown(False, S.TARGET, 1, capi.SAMPLE_S16, x, len(x))
    on = _kernels_shown(True, S.TARGET, 1, capi.SAMPLE_S16, x, len(x))
    assert off == PARENT_KERNELS, off
    assert on == PARENT_KERNELS | AUDIT_KERNELS, on
    d = door("f32p_stereo_48k")
    off = _kernels_shown(False, 48000, 2, capi.SAMPLE_F32P, d["streams"][0], d["frames"][0])
    on = _kernels_shown(True, 48000, 2, capi.SAMPLE_F32P, d["streams"][0], d["frames"][0])
    assert PARENT_KERNELS < off and not off & AUDIT_KERNELS, off
    assert on == off | AUDIT_KERNELS, (on, off)


# ---- 8. state ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,ch,minutes", [(S.TARGET, 1, (1, 3)), (48000, 2, (5, 12))])
def test_state_stays_within_the_new_bound_and_does_not_grow(rate, ch, minutes):
    """include/needle_hip.h: the bound without the audit + 22 rows of 96 B, and the same high-water early and late in a
    stream of one-second chunks.  At 11025 Hz the carried tail repeats every 52 chunks (11025 mod 4 x 1365 = 105 samples
    a second): after 1 and after 3 minutes.  At 48 kHz the resampler's tile phase (period 16 chunks) combines with it to a
    period of 208 chunks, so the high-water of ANY feeder there, audited or not, is complete only after 3.5 minutes: after
    5 and after 12.  Beside it an unaudited feeder fed the same: the audit adds its rows and nothing that grows."""
    bound = S.STATE_BOUND[(rate, ch)] + 22 * 96
    mono = signal(S.TARGET, 80)
    chunk = mono if (rate, ch) == (S.TARGET, 1) else at_rate(mono, rate, ch, 1)
    f, plain = capi.Feeder(1, ch, rate, capi.SAMPLE_S16, 2), capi.Feeder(1, ch, rate, capi.SAMPLE_S16, 2)
    f.set_audit(True)
    state = {}
    for sec in range(60 * minutes[1]):
        f.feed([chunk])
        plain.feed([chunk])
        if sec + 1 in (60 * minutes[0], 60 * minutes[1]):
            state[sec + 1] = (f.state_bytes()[0], plain.state_bytes()[0])
    a = f.audit(0)
    print("state bytes (audited, unaudited)", rate, ch, state, "bound", bound, a)
    assert a["items"] == f.ready(0)[0] > 600 and a["mismatches"] == 0 and a["accepted_mismatches"] == 0
    early, late = state[60 * minutes[0]], state[60 * minutes[1]]
    assert early == late, state
    assert late[0] <= bound and late[1] < late[0] <= late[1] + 22 * 96, (state, bound)
