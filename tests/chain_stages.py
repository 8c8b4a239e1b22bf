"""Tools of tests/test_gpu_chain_stages.py, which looks at what each kernel of the certified fingerprint chain wrote
(needle_hip_fingerprint_stages_debug): the references, the error measures, the numpy statement of the acceptance rule as
features_classify_cert_kernel applies it, the geometry of chunks, and the inputs.  Nothing here needs a device;
tests/test_chain_stages_cpu.py tests these tools themselves."""
import ctypes as C
import os

import numpy as np

from needle_amd import synth
from tests import np_chromaprint as N

HERE = os.path.dirname(os.path.abspath(__file__))
HOP, FRAME = 1365, 4096
SNIPPET = FRAME + 19 * HOP                       # one raw item: 20 frames
U = 2.0 ** -24
ENERGY_SCALE = 16384.0                           # classify_kernels.h kEnergyScale: the kernel's samples carry a factor 1/2
HALF_WINDOW = 0.5 * (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(FRAME) / 4095)) / 32767.0
THR = np.array([c[4:7] for c in N.CLASSIFIERS])  # [16, 3]
COEF = (0.25, 0.75, 1.0, 0.75, 0.25)
GREY = 1e-3                                      # relative width of the band around the radius that float rounding decides


def frames_of(samples):
    return 0 if samples < FRAME else (samples - FRAME) // HOP + 1


def samples_for(frames, extra=0):
    """a stream length of exactly `frames` frames (extra < HOP more samples change nothing); 0 frames: under one frame"""
    return FRAME + HOP * (frames - 1) + extra if frames else 100 + extra


def mono_mix(stereo):
    """AudioProcessor::LoadStereo: (L + R) / 2 with C truncation"""
    total = stereo[0::2].astype(np.int32) + stereo[1::2].astype(np.int32)
    return np.where(total < 0, -((-total) // 2), total // 2).astype(np.int16)


def stereo_of(mono, rng):
    """interleaved L != R whose mix is `mono` exactly: L = m + d, R = m - d"""
    d = rng.integers(1, 4, len(mono)) * rng.choice((-1, 1), len(mono))
    assert np.abs(mono.astype(np.int32)).max(initial=0) + 3 <= 32767
    out = np.empty(2 * len(mono), dtype=np.int16)
    out[0::2] = mono + d
    out[1::2] = mono - d
    return out


# ---- references ---------------------------------------------------------------------------------------------------------
def chroma64(mono):
    """the f64 chroma of one stream, [frames, 12] (numpy, independent of the oracle and of the kernels)"""
    if frames_of(len(mono)) == 0:
        return np.zeros((0, 12))
    return N.chroma_of(mono, np.float64)[0]


def pair_energy(mono):
    """[frames]: sum of squares of the windowed frame in the first pass's units (samples times window / 2), in the pair
    convention of stft_chroma32_kernel: both frames of a pair carry the pair's energy, an absent frame B adds exactly 0."""
    nf = frames_of(len(mono))
    if nf == 0:
        return np.zeros(0)
    own = np.empty(nf)
    for f0 in range(0, nf, 1024):                            # (in slabs: a long stream's frames do not fit at once)
        idx = np.arange(f0, min(nf, f0 + 1024))[:, None] * HOP + np.arange(FRAME)[None, :]
        own[f0: f0 + len(idx)] = ((mono[idx].astype(np.float64) * HALF_WINDOW) ** 2).sum(axis=1)
    pair = own.copy()
    even = np.arange(0, nf - 1, 2)
    pair[even] = pair[even + 1] = own[even] + own[even + 1]
    return pair


_EMU = None


def emu32(mono):
    """stft_chroma32_kernel's per-thread code stepped on the CPU (tests/cpu_emu): chroma [frames, 12], energy [frames, 4]"""
    global _EMU
    if _EMU is None:
        _EMU = C.CDLL(os.path.join(HERE, "cpu_emu", "libemu.so"))
        _EMU.emu_stft_chroma_stream.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    mono = np.ascontiguousarray(mono, dtype=np.int16)
    nf = frames_of(len(mono))
    ch, en = np.zeros((max(nf, 1), 12)), np.zeros((max(nf, 1), 4), dtype=np.float32)
    if nf:
        _EMU.emu_stft_chroma_stream(mono.ctypes.data, len(mono), 1, ch.ctypes.data, en.ctypes.data)
    return ch[:nf], en[:nf]


# ---- the error measures of the first pass ------------------------------------------------------------------------------
def row_errors(c32, c64, e_pair):
    """Per row, max over the classes of |c32 - c64| normalised (1) by the row's largest reference value and (2) by u times
    the pair's total energy in the chroma's units, the quantity S is built on.  Rows of silent pairs (e_pair == 0) are 0
    where c32 is exactly zero and inf elsewhere; a NaN anywhere in a row makes both inf."""
    d = np.abs(c32 - c64).max(axis=1)
    d = np.where(np.isnan(d), np.inf, d)
    silent = e_pair == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        m1 = np.where(silent, np.where(d == 0, 0.0, np.inf), d / c64.max(axis=1))
        m2 = np.where(silent, np.where(d == 0, 0.0, np.inf), d / (U * ENERGY_SCALE * e_pair))
    return m1, m2


def energy_errors(energy4, e_pair):
    """Per row |sum of the four partials / reference - 1|; silent pairs: 0 where every partial is exactly zero, else inf."""
    total = energy4.astype(np.float64).sum(axis=1)
    total = np.where(np.isnan(total), np.inf, total)
    silent = e_pair == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(silent, np.where((energy4 == 0).all(axis=1), 0.0, np.inf), np.abs(total / e_pair - 1.0))


# ---- the acceptance rule -------------------------------------------------------------------------------------------------
def device_rule(chroma, energy4, k, step, norm_clause=True):
    """features_classify_cert_kernel's decision for every kept item of ONE stream, from the first pass's own rows:
    chroma [frames, 12] (f32 values), energy4 [frames, 4] (the partials; pair convention already in them).
    N.classifier_values with the kernel's conventions added: S from kEnergyScale times the folded partials, a row within
    k S (relative) of the 0.01 norm cut makes its items' S infinite, the comparisons are relative (|1 + a - e^t (1 + b)| <=
    e^t (1 + b) (r + r^2), r = k S) and an item with r >= 0.25 is refused.  Returns (refused [kept] bool, bits [kept] u32).
    norm_clause = False: the rule without the norm-cut clause (for showing that a case depends on it)."""
    frames = len(chroma)
    rows = frames - 4
    items = rows - 15
    if items <= 0:
        return np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint32)
    e4 = energy4.astype(np.float32)
    e_frame = ((e4[:, 0] + e4[:, 1]) + (e4[:, 2] + e4[:, 3])).astype(np.float64)
    vals, norm = N.classifier_values(chroma)
    e_row = sum(COEF[j] * e_frame[j:j + rows] for j in range(5))
    n32 = np.maximum(norm.astype(np.float32).astype(np.float64), 1e-30)
    with np.errstate(invalid="ignore", over="ignore"):
        sigma = np.where(e_row > 0, U * np.sqrt(ENERGY_SCALE * e_row / n32), 0.0)
        at_cut = (e_row > 0) & (np.abs(n32 - float(np.float32(0.01))) <= k * sigma * n32 + 1e-9) & norm_clause
        sigma = np.where(at_cut, np.inf, np.where(norm < 0.01, 0.0, sigma))
        x = np.arange(0, items, step)
        r = k * sigma[x[:, None] + np.arange(16)[None, :]].max(axis=1)
        rr = r + r * r
        margin = np.abs(np.expm1(vals[x][:, :, None] - THR[None]))        # |1 + a - e^t (1 + b)| / (e^t (1 + b))
        refused = (margin <= rr[:, None, None]).any(axis=(1, 2)) | ~(r < 0.25)
    q = (vals[x][:, :, None] >= THR[None]).sum(axis=2)
    code = np.array(N.GRAY, dtype=np.uint64)[q]
    bits = np.zeros(len(x), dtype=np.uint64)
    for c in range(16):
        bits = (bits << np.uint64(2)) | code[:, c]
    return refused, bits.astype(np.uint32)


def device_decisions(chroma, energy4, k, step):
    """(refused, grey, bits): `grey` marks the items whose decisive margin lies within GREY (relative) of the radius --
    the rule at (1 - GREY) k and at (1 + GREY) k disagrees (it only refuses more as k grows) -- which float rounding decides."""
    lo, bits = device_rule(chroma, energy4, k * (1.0 - GREY), step)
    hi, _ = device_rule(chroma, energy4, k * (1.0 + GREY), step)
    mid, _ = device_rule(chroma, energy4, k, step)
    assert not (lo & ~hi).any()
    return mid, lo != hi, bits


# ---- geometry ------------------------------------------------------------------------------------------------------------
def chunks_of_item(stream, k, step, chunk_pairs):
    """the chunks (of the batch's global pair index) that kept item k of `stream` spans: frames x .. min(x + 19, frames - 1)"""
    x = k * step
    p0 = stream["pair_base"] + x // 2
    p1 = stream["pair_base"] + min(x + 19, stream["frames"] - 1) // 2
    return range(p0 // chunk_pairs, p1 // chunk_pairs + 1)


def listed_chunks(streams, item_listed, step, chunk_pairs, nchunks):
    """[nchunks] bool: the chunks the listed items' frames span"""
    out = np.zeros(nchunks, dtype=bool)
    for s in streams:
        for k in np.nonzero(item_listed[s["kept_base"]: s["kept_base"] + s["kept"]])[0]:
            out[list(chunks_of_item(s, int(k), step, chunk_pairs))] = True
    return out


def chunk_of_rows(streams, chunk_pairs, frames):
    """[frames]: the chunk every global chroma row lies in"""
    out = np.zeros(frames, dtype=np.int64)
    for s in streams:
        f = np.arange(s["frames"])
        out[s["frame_base"] + f] = (s["pair_base"] + f // 2) // chunk_pairs
    return out


def plan_streams(frames, step, items_per_tile=64):
    """the batch-global numbering of plan_chunk for streams of `frames` frames (what the hook returns as `streams`)"""
    out, fb, pb, kb, tb = [], 0, 0, 0, 0
    for f in frames:
        kept = (max(f - 19, 0) + step - 1) // step
        out.append({"frames": f, "frame_base": fb, "pair_base": pb, "kept": kept, "kept_base": kb, "tile_base": tb})
        fb, pb, kb, tb = fb + f, pb + (f + 1) // 2, kb + kept, tb + (kept + items_per_tile - 1) // items_per_tile
    return out


# ---- the first pass's schedule (stft32_schedule.h stft32_block_range, from the schedule the hook reports) ------------------
def block_range(sched, block, total_pairs):
    x, q, base, size = block & 7, block >> 3, 0, sched["sizes"][0]
    for k in range(3):
        if q < sched["counts"][k]:
            break
        q -= sched["counts"][k]
        base += sched["counts"][k] * sched["sizes"][k]
        size = sched["sizes"][k + 1]
    xfirst = x * sched["pairs_per_xcd"]
    xend = min(xfirst + sched["pairs_per_xcd"], total_pairs)
    f = min(xfirst + base + q * size, xend)
    last = max(min(f + size, xend), f)
    return f, last


def block_class(sched, block):
    q = block >> 3
    for k in range(3):
        if q < sched["counts"][k]:
            return k
        q -= sched["counts"][k]
    return 3


def guided_pairs(compute_units, pairs_per_block=8):
    """the fewest pairs stft32_schedule's guard lets the guided ramp apply to (4 blocks >= 5 slots per XCD, ppb >= 8)"""
    slots_per_xcd = (3 * compute_units + 7) // 8
    blocks = (5 * slots_per_xcd + 3) // 4                    # per XCD, at full size
    return (8 * (blocks - 1)) * pairs_per_block + 1          # ceil(ceil(pairs / ppb) / 8) == blocks first holds here


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def zoo_signal(kind, n, rng):
    """the hostile signals of tests/test_gpu_certified.py's zoo, at any length"""
    t = np.arange(n) / 11025.0
    v = {"strong-5k": lambda: 30 * np.sin(2 * np.pi * 440 * t) + 30000 * np.sin(2 * np.pi * 5000.0 * t),
         "strong-dc": lambda: 300 * np.sin(2 * np.pi * 440 * t) + 30000,
         "square": lambda: np.where(np.sin(2 * np.pi * 220 * t) >= 0, 32767.0, -32768.0),
         "silence": lambda: np.zeros(n),
         "lsb-noise": lambda: rng.standard_normal(n) * 1.0,
         "tone+lsb-noise": lambda: 12000 * np.sin(2 * np.pi * 523.25 * t) + rng.standard_normal(n) * 0.7}[kind]()
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


ZOO = ("strong-5k", "strong-dc", "square", "silence", "lsb-noise")


def audio(seed, n, offset=3000):
    """n samples of a synthetic episode"""
    pcm = synth.make_episode(seed, (offset + n) / 11025.0 + 1.0, 0.0).pcm
    return pcm[offset: offset + n].copy()


def plant(pcm, snippet, k):
    """the 20 frames of `snippet` at sample k x 1365: raw item k of the stream is then the snippet's one item"""
    assert k * HOP + SNIPPET <= len(pcm)
    pcm[k * HOP: k * HOP + SNIPPET] = snippet
    return pcm


# ---- the inputs of the certification test ----------------------------------------------------------------------------------
_NEAR = None


def near_snippets():
    """near-threshold snippets (20 frames, one raw item each) that the first pass cannot decide"""
    global _NEAR
    if _NEAR is None:
        from tests.test_gpu_certified import _near_threshold_pairs
        pairs = _near_threshold_pairs(6, seed=29)
        assert len(pairs) >= 4
        _NEAR = [p for lo, hi, *_ in pairs for p in (lo, hi)]
    return _NEAR


def tile_items(step, env=None):
    """items per tile of the certification's launch: fingerprint.hip tile_items, capped by NEEDLE_HIP_ITEMS_PER_TILE"""
    full = min(64, (63 * 2 + 16 - 16) // step + 1)
    return full if env is None else min(full, env)


CERT_KEPT = lambda ipt: [1, ipt, ipt + 1, 7, 0, 30]          # noqa: E731  kept items of a case's first six streams


def cert_case(step, ipt, near):
    """Streams whose kept counts are 1, a tile, a tile and one, and a ragged mix, a near-threshold snippet as the last item of
    each (a tile's last item, or the only item of its tile); then noise whose feature norms lie under, over and -- the
    last stream, norm_cut_stream -- AT the 0.01 cut."""
    rng = np.random.default_rng(100 * step + ipt)
    streams = []
    for i, n in enumerate(CERT_KEPT(ipt)):
        f = (n - 1) * step + 20 if n else 19
        pcm = audio(700 + 10 * step + i, samples_for(f, extra=int(rng.integers(0, HOP))))
        if n:
            plant(pcm, near[i % len(near)], (n - 1) * step)
        streams.append(pcm)
    for amp in (2.2, 2.6):                                   # feature norms of 0.008 - 0.009 and of 0.011 - 0.013
        streams.append(np.rint(rng.standard_normal(samples_for(19 + 12 * step)) * amp).astype(np.int16))
    streams.append(norm_cut_stream(19 + 12 * step, step))
    return streams


def _row_norm(pcm5):
    """the feature norm of the one FIR row over the five frames of `pcm5`, from the emulated first pass"""
    c = emu32(pcm5)[0]
    fir = sum(COEF[j] * c[j] for j in range(5))
    return float(np.sqrt((fir ** 2).sum()))


NORM_CUT_ROW = 5


def norm_cut_stream(frames, seed, row=NORM_CUT_ROW, dc=150.0):
    """Noise over a DC offset, scaled so that FIR row `row` of the first pass has its norm AT the 0.01 cut: within 1e-4
    (relative), a tenth of K S at K = 64 -- the offset's energy widens S to 1.7e-5.  The items that hold the row (raw items
    up to `row`) are then refused by the norm clause of feature_row_cert whatever their margins, and the rows around it fall
    on either side of the cut.  The scale is found by bisection, then the best of a dither around it (the norm is a
    staircase of the scale at the s16 grid's resolution); a seed whose staircase misses the band is passed over."""
    for attempt in range(8):
        rng = np.random.default_rng(1000 * seed + attempt)
        g = rng.standard_normal(samples_for(frames))
        seg = slice(row * HOP, row * HOP + FRAME + 4 * HOP)
        at = lambda a: _row_norm(np.rint(a * g[seg] + dc).astype(np.int16))                    # noqa: E731
        lo, hi = 0.5, 4.0
        for _ in range(24):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if at(mid) < 0.01 else (lo, mid)
        best = min((lo * (1.0 + u) for u in np.linspace(-3e-3, 3e-3, 401)), key=lambda a: abs(at(a) - 0.01))
        if abs(at(best) - 0.01) < 1e-6:
            return np.rint(best * g + dc).astype(np.int16)
    raise AssertionError("no scale puts the row at the norm cut")
