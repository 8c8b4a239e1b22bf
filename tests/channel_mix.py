"""The channel-mix specification of include/needle_hip.h ("Channel mixes") restated in numpy, for the tests: the default
matrix of a channel mask, the fold-down of C-channel frames to stereo and to mono, and the six-channel test signal.

All arithmetic on the fold-down is integer and exact:
    acc_o  = sum_c coef[o][c] * x_c
    Lo, Ro = clip((acc_o + 16384) >> 15, -32768, 32767)
    mono   = (Lo + Ro) / 2, truncated toward zero
"""
import math
import struct

import numpy as np

from tests.test_sample_formats_cpu import to_s16

# WAVEFORMATEXTENSIBLE / FFmpeg bits, ascending: FL FR FC LFE BL BR FLC FRC BC SL SR -> (weight to L, weight to R)
_H = math.sqrt(0.5)
WEIGHTS = [(1, 0), (0, 1), (_H, _H), (0, 0), (_H, 0), (0, _H), (1, 0), (0, 1), (0.5, 0.5), (_H, 0), (0, _H)]


def default_rows(mask):
    """(left row, right row) of Q15 integers for a channel mask: both rows divided by the larger row sum if that exceeds
    1, then floor(m * 32768 + 0.5)."""
    w = [WEIGHTS[b] for b in range(11) if mask >> b & 1]
    norm = max(1.0, sum(l for l, _ in w), sum(r for _, r in w))
    return ([int(math.floor(l / norm * 32768 + 0.5)) for l, _ in w], [int(math.floor(r / norm * 32768 + 0.5)) for _, r in w])


def fold_stereo(x, left, right):
    """x: interleaved s16 values of len(left) channels -> (Lo, Ro) int16 arrays."""
    c = len(left)
    f = np.asarray(x).astype(np.int64).reshape(-1, c)
    out = []
    for row in (left, right):
        acc = f @ np.asarray(row, dtype=np.int64)
        assert acc.size == 0 or (abs(acc).max() + 16384 < 2 ** 31)
        out.append(np.clip((acc + 16384) >> 15, -32768, 32767))
    return out[0].astype(np.int16), out[1].astype(np.int16)


def stereo_mono(lo, ro):
    """(L + R) / 2 with C truncation toward zero: the stereo path's rule."""
    s = lo.astype(np.int64) + ro.astype(np.int64)
    return (np.sign(s) * (abs(s) // 2)).astype(np.int16)


def fold_mono(x, left, right):
    return stereo_mono(*fold_stereo(x, left, right))


def fold_mono_format(x, left, right, sample_format):
    """Interleaved samples in `sample_format` -> mono s16 under the mix: to_s16 per sample first."""
    return fold_mono(to_s16(x, sample_format), left, right)


def plain_mono(x, channels):
    """(sum of the frame) / channels, truncated toward zero: the plain average."""
    s = np.asarray(x).astype(np.int64).reshape(-1, channels).sum(axis=1)
    return (np.sign(s) * (abs(s) // channels)).astype(np.int16)


def interleave(lo, ro):
    out = np.empty(2 * len(lo), dtype=np.int16)
    out[0::2], out[1::2] = lo, ro
    return out


def six_channel_signal(rate, seconds=12.0, seed=5):
    """5.1 (FL FR FC LFE SL SR, mask 0x60F) as interleaved s16: music in L / R, other notes in C, a 49-82 Hz LFE line and
    quiet surrounds."""
    n = int(rate * seconds)
    t = np.arange(n) / rate
    rng = np.random.default_rng(seed)

    def notes(freqs, every, amp):
        out = np.zeros(n)
        for k in range(int(seconds / every) + 1):
            f = freqs[k % len(freqs)]
            on = (t >= k * every) & (t < (k + 1) * every)
            out[on] = amp * (np.sin(2 * np.pi * f * t[on]) + 0.5 * np.sin(2 * np.pi * 2 * f * t[on]) + 0.25 * np.sin(2 * np.pi * 3 * f * t[on]))
        return out

    left = notes([261.63, 329.63, 392.0, 523.25, 440.0, 349.23], 0.5, 5000) + rng.normal(0, 60, n)
    right = notes([392.0, 523.25, 329.63, 261.63, 349.23, 440.0], 0.5, 5000) + rng.normal(0, 60, n)
    centre = notes([311.13, 466.16, 277.18, 415.3, 369.99], 0.37, 6000)
    lfe = 9000 * np.sin(2 * np.pi * (49 * t + (82 - 49) / (2 * seconds) * t * t))
    sl = notes([233.08, 185.0], 0.9, 500) + rng.normal(0, 30, n)
    sr = notes([207.65, 155.56], 1.1, 500) + rng.normal(0, 30, n)
    x = np.stack([left, right, centre, lfe, sl, sr], axis=1)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16).reshape(-1)


def write_wav(path, pcm, channels, rate, mask=None):
    """Interleaved s16 as RIFF/WAVE: plain PCM, or WAVE_FORMAT_EXTENSIBLE carrying dwChannelMask when `mask` is given."""
    pcm = np.ascontiguousarray(pcm, dtype="<i2")
    base = struct.pack("<HHIIHH", 1 if mask is None else 0xFFFE, channels, rate, rate * channels * 2, channels * 2, 16)
    if mask is not None:  # cbSize, wValidBitsPerSample, dwChannelMask, SubFormat GUID (KSDATAFORMAT_SUBTYPE_PCM)
        base += struct.pack("<HHI", 22, 16, mask) + struct.pack("<IHH", 1, 0, 0x10) + bytes([0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71])
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(base)) + base + b"data" + struct.pack("<I", pcm.nbytes) + pcm.tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
