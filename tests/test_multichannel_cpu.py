"""3-8 channel (surround) input at the host boundary, without a GPU: WAV discovery accepts 3-8 channel files in every
sample format the reader decodes, the multi-GPU plan of a C-channel library is the plan of the mono library of the same
frame counts, and the down-mix entry point is declared and exported."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from needle_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_GUID_TAIL = bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def write_wav_multichannel(path, pcm, channels, rate=11025, kind="s16", extensible=False):
    """RIFF/WAVE writer for interleaved s16 `pcm` in one of the encodings the reader converts back to exactly these
    s16 values: s16, s24 (the reader keeps the top 16 bits) or f32 (scaled by 2^15, rounded); plain or
    WAVE_FORMAT_EXTENSIBLE (sub-format GUID, channel mask 0: the down-mix does not depend on channel order)."""
    x = np.ascontiguousarray(pcm, dtype=np.int16)
    if kind == "s16":
        fmt, bits, payload = 1, 16, x.astype("<i2").tobytes()
    elif kind == "s24":
        w = (x.astype(np.int32) << 8) + 0x5A                    # a low byte the reader drops
        b = w.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]
        fmt, bits, payload = 1, 24, np.ascontiguousarray(b).tobytes()
    elif kind == "f32":
        fmt, bits, payload = 3, 32, (x.astype(np.float32) / np.float32(32768.0)).astype("<f4").tobytes()
    else:
        raise ValueError(kind)
    align = channels * bits // 8
    common = (channels.to_bytes(2, "little") + rate.to_bytes(4, "little") + (rate * align).to_bytes(4, "little")
              + align.to_bytes(2, "little") + bits.to_bytes(2, "little"))
    if extensible:
        body = ((0xFFFE).to_bytes(2, "little") + common + (22).to_bytes(2, "little") + bits.to_bytes(2, "little")
                + (0).to_bytes(4, "little") + fmt.to_bytes(2, "little") + _GUID_TAIL)
    else:
        body = fmt.to_bytes(2, "little") + common
    with open(path, "wb") as f:
        n = len(payload)
        f.write(b"RIFF" + (4 + 8 + len(body) + 8 + n).to_bytes(4, "little") + b"WAVE")
        f.write(b"fmt " + len(body).to_bytes(4, "little") + body)
        f.write(b"data" + n.to_bytes(4, "little") + payload)


def surround(mono, channels, seed):
    """A C-channel signal whose channels differ: the episode's audio in front and centre, noise in the surrounds,
    a low tone on the LFE (channel 3), so that the sum of a frame is not C x the mono sample."""
    rng = np.random.default_rng(seed)
    n = len(mono)
    x = mono.astype(np.int32)
    chans = []
    for c in range(channels):
        if c == 3:
            ch = 3000 * np.sin(2 * np.pi * 55.0 * np.arange(n) / 11025.0)
        elif c in (0, 1, 2):
            ch = x * (0.5 + 0.25 * c) + rng.integers(-200, 200, n)
        else:
            ch = rng.integers(-2500, 2500, n) + (x >> 2)
        chans.append(np.clip(np.rint(ch), -32768, 32767).astype(np.int16))
    return np.stack(chans, axis=1).reshape(-1)


def _cpaths(paths):
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    return C.cast(arr, C.POINTER(C.c_char_p)), arr


def test_header_declares_the_channel_bound_and_the_downmix_entry_point():
    text = open(os.path.join(ROOT, "include", "needle_hip.h")).read()
    m = re.search(r"#define\s+NEEDLE_HIP_MAX_CHANNELS\s+(\d+)", text)
    assert m and int(m.group(1)) == capi.MAX_CHANNELS == 8
    assert "needle_hip_downmix_host" in capi.NEEDLE_HIP_H_SYMBOLS
    assert hasattr(capi.lib(), "needle_hip_downmix_host")
    ffi = open(os.path.join(ROOT, "rust", "needle-hip", "src", "ffi.rs")).read()
    assert "pub fn needle_hip_downmix_host(" in ffi


def test_find_video_files_accepts_3_to_8_channels_in_every_format(tmp_path):
    """Full validation (the WAV header) keeps 3-, 6- and 8-channel files -- 16-bit, 24-bit and float, plain and
    extensible -- and still drops a 9-channel one."""
    L = capi.lib()
    mono = synth.make_episode(0, 2.0, 0.0).pcm
    d = tmp_path / "show"
    d.mkdir()
    want = []
    for ch in (3, 6, 8):
        for kind in ("s16", "s24", "f32"):
            for ext in (False, True):
                name = f"c{ch}-{kind}-{'ext' if ext else 'plain'}.wav"
                write_wav_multichannel(str(d / name), surround(mono, ch, ch), ch, kind=kind, extensible=ext)
                want.append(name)
    for name, ext in (("z9-plain.wav", False), ("z9-ext.wav", True)):
        write_wav_multichannel(str(d / name), surround(mono, 9, 9), 9, extensible=ext)
    ptr, keep = _cpaths([str(d)])
    videos = C.POINTER(C.c_char_p)()
    n = C.c_size_t(0)
    assert L.needle_util_find_video_files(ptr, 1, True, True, C.byref(videos), C.byref(n)) == 0
    got = [os.path.basename(videos[i].decode()) for i in range(n.value)]
    L.needle_util_video_files_free(videos, n)
    assert got == sorted(want)
    # without full validation every .wav is listed, the 9-channel files included
    assert L.needle_util_find_video_files(ptr, 1, False, True, C.byref(videos), C.byref(n)) == 0
    assert n.value == len(want) + 2
    L.needle_util_video_files_free(videos, n)


@pytest.mark.parametrize("endings", [False, True])
def test_rank_plan_of_a_multichannel_library_is_the_mono_plan(endings):
    """needle_hip_library_rank_videos is a pure function of the frame counts: num_values = frames x C (plus a partial
    frame, which is dropped) gives, for every C in 3..8, world size and rank, the plan of the mono library."""
    rng = np.random.default_rng(4)
    frames = [int(f) for f in rng.integers(11025 * 60, 11025 * 1500, 29)] + [0, 11025 * 3]
    lib = capi.Library(len(frames))
    if endings:
        lib.include_endings(0.25)
    for world in (1, 2, 3, 8):
        for rank in range(world):
            mono = lib.rank_videos(frames, world, rank, channels=1)
            for ch in range(3, 9):
                lens = [f * ch + (k % ch) for k, f in enumerate(frames)]
                assert lib.rank_videos(lens, world, rank, channels=ch) == mono, (world, rank, ch)
    with pytest.raises(capi.NeedleError):
        lib.rank_videos([f * 9 for f in frames], 2, 0, channels=9)
    with pytest.raises(capi.NeedleError):
        lib.rank_videos(frames, 2, 0, channels=0)
