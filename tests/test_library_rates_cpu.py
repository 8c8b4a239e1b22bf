"""Library PCM at any sample rate, without a GPU: needle_hip_library_set_sample_rate is declared, exported and bound in
Rust, refuses what it must, and the multi-GPU plan of a library at 44.1 / 48 kHz is the one a small model of the
windows computes (cut at the source rate, kept hashes from the resampled length, equal flat blocks of the arena)."""
import os

import numpy as np
import pytest

from needle_amd import capi
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = O.NS
ERR = {name: i for i, name in enumerate(capi.ERROR_NAMES)}


def test_setter_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "needle_hip.h")).read()
    assert "enum NeedleError needle_hip_library_set_sample_rate(NeedleHipLibrary *library, int sample_rate);" in text
    assert "needle_hip_library_set_sample_rate" in capi.NEEDLE_HIP_H_SYMBOLS
    assert hasattr(capi.lib(), "needle_hip_library_set_sample_rate")
    ffi = open(os.path.join(ROOT, "rust", "needle-hip", "src", "ffi.rs")).read()
    assert "pub fn needle_hip_library_set_sample_rate(library: *mut NeedleHipLibrary, sample_rate: c_int) -> NeedleError;" in ffi
    assert "pub fn set_sample_rate(" in open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")).read()


def test_setter_errors():
    L = capi.lib()
    assert L.needle_hip_library_set_sample_rate(None, 11025) == ERR["NullArgument"]
    lib = capi.Library(3)
    for bad in (0, 1999, 768001, -48000):
        assert L.needle_hip_library_set_sample_rate(lib._h, bad) == ERR["InvalidArgument"], bad
    for good in (2000, 11025, 48000, 768000):
        assert L.needle_hip_library_set_sample_rate(lib._h, good) == ERR["Ok"], good
    assert lib.set_sample_rate(44100) is lib                                  # chainable, like include_endings
    with pytest.raises(capi.NeedleError):
        lib.set_sample_rate(1999)


def _model_rank_videos(frames, rate, endings, world, rank, opening=0.5, ending=0.25, hash_duration=0.3):
    """library.cpp's plan restated: windows cut at `rate` (Analyzer::windows), kept hashes of the 11025 Hz resident
    window, stride of whole 64-hash tiles with rows * tiles a multiple of the world size, and the videos whose rows the
    rank's flat block meets with a kept column (for_rows_of_block)."""
    L = capi.lib()
    hd = O.duration_from_secs_f32(hash_duration)
    step = (hd // 1_000_000) // O.item_duration_ms()
    R = 2 if endings else 1
    kept = []
    for f in frames:
        dur = O.duration_from_secs_f64(f * (1.0 / rate))
        n_open = min(O.duration_mul_f32(dur, opening) * rate // NS, f)
        seek = O.duration_mul_f32(dur, float(np.float32(1.0) - np.float32(ending)))
        first = min(seek * rate // NS, f)
        for count in [n_open] + ([f - first] if endings else []):
            resident = count if rate == 11025 else L.needle_hip_resample_out_len(count, rate)
            kept.append(L.needle_hip_fingerprint_num_kept(resident, step))
    rows = len(kept)
    tiles = max(1, (max(kept) + 63) // 64)
    while world > 1 and (rows * tiles) % world:
        tiles += 1
    stride = 64 * tiles
    if world == 1:
        return 0, len(frames)
    block = rows * stride // world
    begin, end = rank * block, (rank + 1) * block
    lo, hi = len(frames), 0
    row = begin // stride
    while row < rows and row * stride < end:
        r0 = row * stride
        c0 = begin - r0 if begin > r0 else 0
        c1 = min(end - r0, stride, kept[row])
        if c0 < c1:
            lo, hi = min(lo, row // R), max(hi, row // R + 1)
        row += 1
    return (lo, hi - lo) if lo < hi else (0, 0)


def _frames(rate, seed):
    """28 episodes of 21-25 minutes at `rate`, a few of them very short, so that blocks end inside and between rows."""
    rng = np.random.default_rng(seed)
    f = [int(rng.integers(21 * 60 * rate, 25 * 60 * rate)) for _ in range(28)]
    f[3], f[17] = 7 * rate + 13, 61 * rate
    return f


@pytest.mark.parametrize("rate", [44100, 48000])
@pytest.mark.parametrize("endings", [False, True])
def test_rank_videos_at_a_rate_equals_the_model(rate, endings):
    frames = _frames(rate, rate + endings)
    for ch in (1, 2, 6):
        lens = [f * ch + (1 if ch > 1 and k % 5 == 0 else 0) for k, f in enumerate(frames)]  # (a partial frame is dropped)
        lib = capi.Library(len(frames))
        if endings:
            lib.include_endings(0.25)
        lib.set_sample_rate(rate)
        for world in range(1, 9):
            for rank in range(world):
                assert lib.rank_videos(lens, world, rank, channels=ch) == \
                    _model_rank_videos(frames, rate, endings, world, rank), (rate, endings, ch, world, rank)


@pytest.mark.parametrize("endings", [False, True])
def test_rank_videos_at_11025_is_the_default(endings):
    frames = _frames(11025, 7 + endings)
    lens = [2 * f for f in frames]
    plain, explicit = capi.Library(len(frames)), capi.Library(len(frames)).set_sample_rate(11025)
    if endings:
        plain.include_endings(0.25)
        explicit.include_endings(0.25)
    for world in range(1, 9):
        for rank in range(world):
            got = explicit.rank_videos(lens, world, rank, channels=2)
            assert got == plain.rank_videos(lens, world, rank, channels=2)
            assert got == _model_rank_videos(frames, 11025, endings, world, rank)

