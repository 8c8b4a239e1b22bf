"""Channel mixes without a device: the default matrices as literals, every refusal of include/needle_hip.h "Channel
mixes" (each made on the host, before any device is asked for), the three surfaces agreeing, and wav_probe's channel
mask as the file analyzer sees it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from needle_amd import capi
from tests import channel_mix as M
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["needle_hip_channel_mix_default", "needle_hip_rematrix_host", "needle_hip_analyzer_set_channel_mix",
           "needle_hip_analyzer_set_layout_downmix", "needle_hip_comparator_set_layout_downmix",
           "needle_hip_library_set_channel_mix", "needle_hip_feeder_set_lane_mix"]
INVALID, NULL = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("NullArgument")

# include/needle_hip.h: mask -> (left row, right row)
DEFAULTS = {
    0x3: ([32768, 0], [0, 32768]),                                                           # stereo: the identity
    0x4: ([23170], [23170]),                                                                 # FC alone: sqrt(1/2) to both
    0x7: ([19195, 0, 13573], [0, 19195, 13573]),                                             # 3.0
    0x33: ([19195, 0, 13573, 0], [0, 19195, 0, 13573]),                                      # quad
    0x107: ([14847, 0, 10498, 7423], [0, 14847, 10498, 7423]),                               # 4.0
    0x3F: ([13573, 0, 9598, 0, 9598, 0], [0, 13573, 9598, 0, 0, 9598]),                      # 5.1 back
    0x60F: ([13573, 0, 9598, 0, 9598, 0], [0, 13573, 9598, 0, 0, 9598]),                     # 5.1 side
    0x70F: ([11244, 0, 7951, 0, 5622, 7951, 0], [0, 11244, 7951, 0, 5622, 0, 7951]),         # 6.1
    0x63F: ([10498, 0, 7423, 0, 7423, 0, 7423, 0], [0, 10498, 7423, 0, 0, 7423, 0, 7423]),   # 7.1
}
FIVE_ONE = capi.ChannelMix.of(*DEFAULTS[0x60F])


def raises(code, f, *args, **kw):
    with pytest.raises(capi.NeedleError) as e:
        f(*args, **kw)
    assert e.value.code == code, (e.value, code)


def test_default_matrices_are_the_pinned_literals():
    for mask, (left, right) in DEFAULTS.items():
        m = capi.channel_mix_default(mask)
        assert m.channels == len(left) == bin(mask).count("1")
        assert m.rows() == (left, right), (hex(mask), m.rows())
        assert M.default_rows(mask) == (left, right), hex(mask)                # the numpy helper states the same rule
        assert list(m.coef[0][m.channels:]) == [0] * (8 - m.channels)
    assert sum(DEFAULTS[0x60F][0]) == 32769                                    # full-scale 5.1 input clips
    # stereo under the identity is the existing (L + R) / 2
    x = np.array([-1, 0, -3, -4, 32767, 32767, -32768, -32768, 5, -8], np.int16)
    assert M.fold_mono(x, *DEFAULTS[0x3]).tolist() == M.plain_mono(x, 2).tolist() == [0, -3, 32767, -32768, -1]


def test_default_refuses_bad_masks_and_null():
    L = capi.lib()
    out = capi.ChannelMix.of([7] * 3, [9] * 3)
    for mask in (0, 0x800, 0x1000, 0x80000000, 0x803, 0x7FF, 0x3FF, 0x1FF):   # no bit; a bit above 0x400; popcount 11, 10, 9
        assert L.needle_hip_channel_mix_default(mask, C.byref(out)) == INVALID, hex(mask)
        assert out.rows() == ([7] * 3, [9] * 3)                                # untouched
    assert L.needle_hip_channel_mix_default(0xFF, C.byref(out)) == 0 and out.channels == 8                 # popcount 8 is the limit
    assert L.needle_hip_channel_mix_default(0x3, None) == NULL


def _bad_mixes():
    ok = DEFAULTS[0x60F]
    return {
        "channels 0": capi.ChannelMix.of(*ok, channels=0),
        "channels 9": capi.ChannelMix.of([1] * 8, [1] * 8, channels=9),
        "channels -1": capi.ChannelMix.of(*ok, channels=-1),
        "coefficient 32769": capi.ChannelMix.of([32769, 0], [0, 1]),
        "coefficient -32769": capi.ChannelMix.of([0, 1], [-32769, 0]),
        "row sum 65536": capi.ChannelMix.of([32768, 32767, 1], [0, 0, 0]),
        "row sum 65536, signed": capi.ChannelMix.of([0, 0, 0], [-32768, 32767, -1]),
    }


def test_limits_of_a_mix_are_refused_by_every_setter():
    L = capi.lib()
    at_the_bound = capi.ChannelMix.of([32768, -32767], [-32768, 32767])        # sum |coef| = 65535: the most that is allowed
    for name, bad in _bad_mixes().items():
        a = capi.Analyzer(["a.wav"]).set_channel_mix(FIVE_ONE)
        raises(INVALID, a.set_channel_mix, bad)
        assert a._mix is FIVE_ONE, name                                        # unchanged
        lib = capi.Library(2)
        lib.set_channel_mix(at_the_bound)
        raises(INVALID, lib.set_channel_mix, bad)
        f = capi.Feeder.with_formats([(bad.channels if 1 <= bad.channels <= 8 else 6, 48000, capi.SAMPLE_S16)] * 2)
        if bad.channels != 0:                                                  # (0 means "no mix" in an array of mixes)
            raises(INVALID, f.set_lane_mix, [0], [bad])
            out = np.zeros(4, np.int16)
            fmt = capi._lane_formats([(max(1, min(bad.channels, 8)), 48000, capi.SAMPLE_S16)])
            ptr, n, o = (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(0), (C.c_void_p * 1)(out.ctypes.data)
            assert L.needle_hip_rematrix_host(ptr, n, fmt, C.byref(bad), 1, o) == INVALID, name
    capi.Analyzer(["a.wav"]).set_channel_mix(at_the_bound).set_channel_mix(None)
    capi.Feeder.with_formats([(2, 48000, capi.SAMPLE_F32)]).set_lane_mix([0], [at_the_bound])


def test_channel_count_mismatch_per_driver():
    pcm = np.zeros(8 * 6, np.int16)
    a = capi.Analyzer(["a.wav"]).set_channel_mix(FIVE_ONE)
    raises(INVALID, a.run_pcm, [pcm], channels=2)
    raises(INVALID, a.run_pcm, [pcm.astype(np.float32)], channels=3, sample_format=capi.SAMPLE_F32)
    lib = capi.Library(2).set_channel_mix(FIVE_ONE)
    raises(INVALID, lib.set_pcm, [pcm, pcm], [pcm.size] * 2, channels=2)
    L = capi.lib()
    ptrs, lens = (C.c_void_p * 2)(pcm.ctypes.data, pcm.ctypes.data), (C.c_size_t * 2)(pcm.size, pcm.size)
    assert L.needle_hip_library_stream_pcm(lib._h, ptrs, lens, 8) == INVALID
    L.needle_hip_library_set_pcm_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int]
    assert L.needle_hip_library_set_pcm_device(lib._h, ptrs, lens, 5) == INVALID
    f = capi.Feeder.with_formats([(2, 44100, capi.SAMPLE_S16), (6, 48000, capi.SAMPLE_S16)])
    raises(INVALID, f.set_lane_mix, [1, 0], [FIVE_ONE, FIVE_ONE])              # lane 0 is stereo ...
    raises(INVALID, f.set_lane_mix, [2], [FIVE_ONE])                           # ... and there is no lane 2
    f.set_lane_mix([1, 0], [FIVE_ONE, None])
    out = np.zeros(8, np.int16)
    fmt = capi._lane_formats([(2, 48000, capi.SAMPLE_S16)])
    ptr, n, o = (C.c_void_p * 1)(pcm.ctypes.data), (C.c_size_t * 1)(16), (C.c_void_p * 1)(out.ctypes.data)
    assert L.needle_hip_rematrix_host(ptr, n, fmt, C.byref(FIVE_ONE), 1, o) == INVALID and not out.any()


def test_feeder_new_refuses_lane_mixes_and_null_arguments():
    L = capi.lib()
    f = capi.Feeder(2, channels=6, sample_rate=48000)
    raises(INVALID, f.set_lane_mix, [0], [FIVE_ONE])                           # as it refuses reset_format
    g = capi.Feeder.with_formats([(6, 48000, capi.SAMPLE_S16)])
    lanes, mixes = (C.c_size_t * 1)(0), capi._channel_mixes([FIVE_ONE])
    assert L.needle_hip_feeder_set_lane_mix(None, lanes, mixes, 1) == NULL
    assert L.needle_hip_feeder_set_lane_mix(g._h, None, mixes, 1) == NULL
    assert L.needle_hip_feeder_set_lane_mix(g._h, lanes, None, 1) == NULL
    assert L.needle_hip_analyzer_set_channel_mix(None, C.byref(FIVE_ONE)) == NULL
    assert L.needle_hip_analyzer_set_layout_downmix(None, True) == NULL
    assert L.needle_hip_comparator_set_layout_downmix(None, True) == NULL
    assert L.needle_hip_library_set_channel_mix(None, C.byref(FIVE_ONE)) == NULL
    out = np.zeros(4, np.int16)
    fmt = capi._lane_formats([(6, 48000, capi.SAMPLE_S16)])
    ptr, n, o = (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(0), (C.c_void_p * 1)(out.ctypes.data)
    for args in [(None, n, fmt, mixes, 1, o), (ptr, None, fmt, mixes, 1, o), (ptr, n, None, mixes, 1, o), (ptr, n, fmt, None, 1, o),
                 (ptr, n, fmt, mixes, 1, None)]:
        assert L.needle_hip_rematrix_host(*args) == NULL
    assert L.needle_hip_rematrix_host(ptr, n, fmt, mixes, 1, o) == 0           # no whole frame: nothing to do, no device asked for


def test_symbols_and_struct_in_every_layer(tmp_path):
    header = R.strip_comments(open(os.path.join(ROOT, "include", "needle_hip.h")).read())
    ffi_rs = open(os.path.join(ROOT, "rust", "needle-hip", "src", "ffi.rs")).read()
    protos = R.c_prototypes()
    fns, _, _ = R.rust_declarations()
    L = capi.lib()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in capi.NEEDLE_HIP_H_SYMBOLS and hasattr(L, sym), sym
        assert fns[sym] == protos[sym], (sym, fns[sym], protos[sym])
    # the struct: 4 + 2 * 8 * 4 bytes, coef behind channels, in C, ctypes and Rust
    src = os.path.join(str(tmp_path), "layout.c")
    open(src, "w").write('#include <stddef.h>\n#include <stdio.h>\n#include "needle_hip.h"\nint main(void) {\n'
                         '  printf("%zu %zu %zu\\n", sizeof(NeedleHipChannelMix), offsetof(NeedleHipChannelMix, channels),'
                         ' offsetof(NeedleHipChannelMix, coef));\n  return 0;\n}\n')
    exe = os.path.join(str(tmp_path), "layout")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["68", "0", "4"]
    assert (C.sizeof(capi.ChannelMix), capi.ChannelMix.channels.offset, capi.ChannelMix.coef.offset) == (68, 0, 4)
    body = re.search(r"#\[repr\(C\)\]\s*(?:#\[[^\]]*\]\s*)*pub struct NeedleHipChannelMix\s*\{(.*?)\}", ffi_rs, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*:\s*([^,]+),", body) == [("channels", "i32"), ("coef", "[[i32; 8]; 2]")]


def test_wav_probe_reads_the_channel_mask(tmp_path):
    """tests/cpp/wav_mask.cpp prints what wav_probe makes of a header: dwChannelMask (bytes 20-23 of the fmt chunk) of a
    WAVE_FORMAT_EXTENSIBLE file, 0 of a plain one; everything else it reads stays what it was."""
    pcm = M.six_channel_signal(11025, 0.5)
    names = {"ext.wav": (6, 0x60F), "back.wav": (6, 0x3F), "plain.wav": (6, None), "zero.wav": (6, 0), "stereo.wav": (2, 0x3)}
    paths = []
    for name, (channels, mask) in names.items():
        paths.append(os.path.join(str(tmp_path), name))
        M.write_wav(paths[-1], pcm[: pcm.size // 6 * channels], channels, 11025, mask=mask)
    raw = open(paths[0], "rb").read()
    at = raw.index(b"fmt ") + 8
    assert int.from_bytes(raw[at + 20: at + 24], "little") == 0x60F and int.from_bytes(raw[at: at + 2], "little") == 0xFFFE
    exe = os.path.join(str(tmp_path), "wav_mask")
    lib_dir = os.path.dirname(capi.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "needle_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "wav_mask.cpp"), "-L", lib_dir, "-lneedle_capi", "-Wl,-rpath," + lib_dir], check=True)
    out = subprocess.run([exe] + paths + [os.path.join(str(tmp_path), "missing.wav")], capture_output=True, text=True, check=True)
    assert out.stdout.split("\n")[:-1] == ["6 11025 16 0x60F", "6 11025 16 0x3F", "6 11025 16 0x0", "6 11025 16 0x0", "2 11025 16 0x3",
                                          "error"], out.stdout + out.stderr
