"""The resampler's kernel plans, for tests/test_resample_plan_cpu.py and tests/test_gpu_resample_plans.py: the class of a
plan (which kernel, which instantiation, which branch of its geometry), the table of rates the GPU test resamples -- one
of every class the planner can select with the default environment, the CPU test proves it -- and the streams and the
signal of a case, derived from the plan.  No device."""
import numpy as np

from needle_amd import capi

TARGET = 11025
LO, HI = 2000, 768000                      # the rates the product accepts


def _count(k):
    return "1" if k == 1 else "2" if k == 2 else ">=3"


def class_key(p):
    """The class of a plan (capi.resample_plan's dict, or a row of capi.resample_plans): the family, then every flag and
    bucket that selects another instantiation or another branch of the kernel.  Workgroups per tile count as 1 / 2 / >=3,
    multiplying waves as 10 / <10."""
    f = p["family"]
    f = f if isinstance(f, str) else capi.RESAMPLE_FAMILIES[int(f)]
    if f == "mfma":
        return (f, "steps%d" % p["mfma_steps"], "long-row" if p["mf_long_row"] else "rows-fit",
                "splits" + _count(p["mf_splits"]), "waves10" if p["mf_waves"] == 10 else "waves<10")
    if f == "quad":
        return (f, "vec4" if p["vec4"] else "scalar", "small" if p["quad_small"] else "large",
                "splits" + _count(p["quad_splits"]), "rounds%d" % p["quad_rounds"])
    if f == "general":
        return (f, "row" if p["row_mode"] else "contiguous", "rows-in-lds" if p["rows_in_lds"] else "global",
                "vec4" if p["vec4"] else "scalar", "n%d" % p["n"])
    if f == "dec":
        return (f, "q%d" % p["dec_q"])
    return (f,)


# One rate of every class, the one with the smallest L x T (so that a design's tables stay small; the CPU test prints the
# census these came from), in the census's order ...
CHEAPEST = [
    44100, 22050,                                                     # dec
    2205, 2835, 2030, 3675, 2625, 2175, 33075, 2450, 2058,            # general, contiguous, global
    543900, 617400, 529200, 714420,                                   # ... with M % 4 == 0
    8820, 2520, 14700, 2100, 2400, 4900, 2352,                        # general, contiguous, rows in LDS
    642929, 602070, 721917, 713475,                                   # general, row, global: n = 1, 2, 4, 8
    643076, 603120, 721476, 718200,                                   # ... with M % 4 == 0
    11025,                                                            # identity
    4800, 9408, 2240, 4032, 2000, 2184,                               # mfma, 12 steps
    11100, 14400, 11060, 11088, 11300, 11256,                         # mfma, 20 steps
    19200, 28224, 18760, 18648, 18700, 18732,                         # mfma, 36 steps
    33900, 35700, 33880, 33768, 33800, 33852,                         # mfma, 52 steps, rows fit
    36300,                                                            # mfma, 52 steps, long rows
    102375, 9849, 4875, 141120, 48804, 48900,                         # quad
]
# ... and the rates users have: decoder rates, NTSC pull-down, CD-ROM XA, the classic Mac, one above the target, the
# smallest general one, and the largest accepted rate coprime to 11025 (the CPU test finds it by its sweep)
USER_RATES = [384000, 352800, 705600, 64000, 50000, 47952, 37800, 22254, 11024, 7350, 29896]
RATES = CHEAPEST + USER_RATES


def stream_lengths(p):
    """Samples per channel of the streams of one call, from the plan: a tile is tile_outputs outputs = tile_outputs / L
    * M inputs.  Long streams with the empty and the short ones between them: three tiles, nothing, exactly one tile, one
    sample, three tiles + 1 sample, T / 2 - 1 samples (every tap window hangs over both ends), and two tiles plus a
    ragged tail whose last output lies inside a block of sixteen outputs and inside a quad of four."""
    L, M, T, tile = p["L"], p["M"], p["T"], p["tile_outputs"]
    assert tile % L == 0
    tile_in = tile // L * M
    want = 2 * tile + min(54, tile - 1)
    ragged = None
    for n_in in range(want * M // L, 2 * tile_in, -1):
        if (n_in * L + M - 1) // M % 4 != 0:                       # (then not a multiple of 16 either)
            ragged = n_in
            break
    if ragged is None:                                             # a tile of one or two outputs has no ragged end
        ragged = 2 * tile_in + 1
    return [3 * tile_in, 0, tile_in, 1, 3 * tile_in + 1, max(T // 2 - 1, 0), ragged]


def stretch_of(n, p):
    """[a, b): the samples of a stream of n that hold the full-scale stretch: 64 outputs' worth in the middle."""
    w = min(n // 2, -(-64 * p["M"] // p["L"]))
    a = (n - w) // 2
    return a, a + w


def signal(n, ch, p, seed):
    """Interleaved s16 of n samples per channel at the plan's rate: a sine plus noise at about half scale, and in the
    middle one stretch of full-scale alternation slow enough to pass the filter (half a period is eight outputs), whose
    overshoot reaches the clamp on both sides.  Stereo: left and right differ by thousands, their sum is odd about half
    the time and negative about half the time, so the truncating down-mix matters; in the stretch both are full scale."""
    rng = np.random.default_rng(seed)
    per_out = p["M"] / p["L"]                                      # input samples per output
    t = np.arange(n)
    m = 11000 * np.sin(2 * np.pi * t / (per_out * (23.0 + seed % 7))) + 4500 * rng.standard_normal(n)
    m = np.clip(np.rint(m), -16000, 16000).astype(np.int64)
    a, b = stretch_of(n, p)
    hp = max(int(round(8 * per_out)), 2)
    square = np.where((t // hp) % 2 == 0, 32767, -32768)
    if ch == 1:
        m[a:b] = square[a:b]
        return m.astype(np.int16)
    d = rng.integers(-8000, 8000, n)
    left, right = m + d, m - d + rng.integers(0, 2, n)             # left + right = 2 m + (0 or 1)
    left[a:b] = square[a:b]
    right[a:b] = square[a:b]
    return np.stack([left, right], axis=1).astype(np.int16).reshape(-1)


def check_reference(ref, n_in, p):
    """The conditions on the inputs, checked on the oracle's output of one stream: it is not constant, it reaches the
    clamp on both sides where the stream has the full-scale stretch, and fewer than 1 % of the outputs outside the
    stretch are clamped."""
    ref = np.asarray(ref, dtype=np.int64)
    if len(ref) < 64:
        return
    assert ref.min() != ref.max(), "constant output"
    a, b = stretch_of(n_in, p)
    reach = 17 if p["M"] >= p["L"] else -(-17 * p["L"] // p["M"])    # outputs a sample's taps reach: 16 zero crossings
    oa = max(a * p["L"] // p["M"] - reach, 0)
    ob = min(-(-b * p["L"] // p["M"]) + reach, len(ref))
    clamped = (ref == 32767) | (ref == -32768)
    if b - a >= 48 * p["M"] // p["L"]:                             # the whole stretch fits the stream
        assert (ref[oa:ob] == 32767).any() and (ref[oa:ob] == -32768).any(), "the clamp is not reached"
    outside = np.concatenate([clamped[:oa], clamped[ob:]])
    assert outside.sum() < 0.01 * max(len(outside), 1), "clamped outside the full-scale stretch"
