"""The streaming fingerprinter's boundary without a GPU: the ten needle_hip_feeder_* symbols through every layer, the
argument errors (checked before any device work), the host arithmetic of needle_hip_feeder_num_ready against the
one-shot count and the documented lag, and the loud failure when there is no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from needle_amd import capi
from tests import rust_ffi_check as R
from tests.test_gpu_library_rates import FAMILIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["needle_hip_feeder_new", "needle_hip_feeder_free", "needle_hip_feeder_feed", "needle_hip_feeder_finish",
           "needle_hip_feeder_reset", "needle_hip_feeder_ready", "needle_hip_feeder_items", "needle_hip_feeder_frame_hashes",
           "needle_hip_feeder_state_bytes", "needle_hip_feeder_num_ready"]
# include/needle_hip.h: the unfinished count lags the one-shot's by at most L raw items, ceil(L / step) kept ones
LAG = {11025: 1, 44100: 2, 22050: 3, 48000: 3, 96000: 3, 32000: 7, 12345: 10}
INVALID, NULL = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("NullArgument")


def test_symbols_in_every_layer():
    header = R.strip_comments(open(os.path.join(ROOT, "include", "needle_hip.h")).read())
    lib_rs = open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")).read()
    protos = R.c_prototypes()
    fns, _, _ = R.rust_declarations()
    L = capi.lib()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(L, sym), sym
        assert sym in capi.NEEDLE_HIP_H_SYMBOLS, sym
        assert sym in fns, f"{sym} is not declared in ffi.rs"
        assert fns[sym] == protos[sym], (sym, fns[sym], protos[sym])
        assert "ffi::%s(" % sym in lib_rs, f"{sym} is not used by lib.rs"
    assert "typedef struct NeedleHipFeeder NeedleHipFeeder;" in header


def _new(lanes=1, channels=1, rate=11025, fmt=capi.SAMPLE_S16, step=1, out=True):
    h = C.c_void_p()
    code = capi.lib().needle_hip_feeder_new(lanes, channels, rate, fmt, step, C.byref(h) if out else None)
    return code, h


def test_argument_errors():
    L = capi.lib()
    assert _new(out=False)[0] == NULL
    assert _new(lanes=0)[0] == INVALID
    assert _new(channels=0)[0] == INVALID and _new(channels=9)[0] == INVALID
    assert _new(fmt=10)[0] == INVALID and _new(fmt=-1)[0] == INVALID
    assert _new(rate=1999)[0] == INVALID and _new(rate=768001)[0] == INVALID
    assert _new(step=0)[0] == INVALID
    for ch, rate, fmt in [(1, 11025, capi.SAMPLE_S16), (8, 768000, capi.SAMPLE_F64P), (2, 2000, capi.SAMPLE_U8)]:
        code, h = _new(3, ch, rate, fmt, 2)
        assert code == 0 and h.value
        L.needle_hip_feeder_free(h)
    L.needle_hip_feeder_free(None)

    code, h = _new(2, 2)
    assert code == 0
    pcm = np.zeros(64, dtype=np.int16)
    ptrs = (C.c_void_p * 2)(pcm.ctypes.data, pcm.ctypes.data)
    lens = (C.c_size_t * 2)(0, 0)
    kept, fed, fin = C.c_size_t(7), C.c_uint64(7), C.c_bool(True)
    assert L.needle_hip_feeder_feed(None, ptrs, lens) == NULL
    assert L.needle_hip_feeder_feed(h, None, lens) == NULL and L.needle_hip_feeder_feed(h, ptrs, None) == NULL
    assert L.needle_hip_feeder_finish(None, None, 0) == NULL and L.needle_hip_feeder_reset(None, None, 0) == NULL
    assert L.needle_hip_feeder_ready(None, 0, C.byref(kept), C.byref(fed), C.byref(fin)) == NULL
    assert L.needle_hip_feeder_items(None, 0, 0, 0, None) == NULL
    assert L.needle_hip_feeder_state_bytes(None, (C.c_uint64 * 2)()) == NULL and L.needle_hip_feeder_state_bytes(h, None) == NULL
    out = C.c_void_p()
    assert L.needle_hip_feeder_frame_hashes(None, 0, 1, 0, 0.3, b"", C.byref(out)) == NULL
    assert L.needle_hip_feeder_frame_hashes(h, 0, 1, 0, 0.3, b"", None) == NULL
    # a lane out of range
    bad = (C.c_size_t * 1)(2)
    assert L.needle_hip_feeder_finish(h, bad, 1) == INVALID and L.needle_hip_feeder_reset(h, bad, 1) == INVALID
    assert L.needle_hip_feeder_ready(h, 2, C.byref(kept), C.byref(fed), C.byref(fin)) == INVALID
    assert L.needle_hip_feeder_items(h, 2, 0, 0, None) == INVALID
    # a partial frame in ANY lane: nothing is consumed, whatever the other lanes hold
    lens = (C.c_size_t * 2)(64, 63)
    assert L.needle_hip_feeder_feed(h, ptrs, lens) == INVALID
    # a null chunk with a length
    nptrs = (C.c_void_p * 2)(pcm.ctypes.data, None)
    lens = (C.c_size_t * 2)(0, 64)
    assert L.needle_hip_feeder_feed(h, nptrs, lens) == NULL
    # an empty feed needs no device and changes nothing
    lens = (C.c_size_t * 2)(0, 0)
    assert L.needle_hip_feeder_feed(h, ptrs, lens) == 0
    assert L.needle_hip_feeder_ready(h, 1, C.byref(kept), C.byref(fed), C.byref(fin)) == 0
    assert (kept.value, fed.value, fin.value) == (0, 0, False)
    # items beyond what is there; frame hashes of unfinished lanes; a hash duration that asks for another step
    assert L.needle_hip_feeder_items(h, 0, 0, 1, (C.c_uint32 * 1)()) == INVALID
    assert L.needle_hip_feeder_frame_hashes(h, 0, 1, 0, 0.3, b"", C.byref(out)) == INVALID     # step 1 is not 0.3 s
    assert L.needle_hip_feeder_frame_hashes(h, 0, 1, 0, 0.0, b"", C.byref(out)) == capi.ERROR_NAMES.index("AnalyzerInvalidHashDuration")
    sb = (C.c_uint64 * 2)()
    assert L.needle_hip_feeder_state_bytes(h, sb) == 0 and sb[0] == 0 and sb[1] == 0
    L.needle_hip_feeder_free(h)
    code, h = _new(2, 1, step=2)
    assert L.needle_hip_feeder_frame_hashes(h, 0, 1, 0, 0.3, b"", C.byref(out)) == INVALID     # right step, unfinished lanes
    L.needle_hip_feeder_free(h)


def _one_shot(n, rate, step):
    L = capi.lib()
    return int(L.needle_hip_fingerprint_num_kept(int(L.needle_hip_resample_out_len(n, rate)), step))


@pytest.mark.parametrize("rate", sorted({r for r, _ in FAMILIES} | {11025}))
@pytest.mark.parametrize("step", [1, 2, 3])
def test_num_ready_is_monotone_exact_when_finished_and_lags_by_at_most_l(rate, step):
    bound = -(-LAG[rate] // step)
    prev, n = 0, 0
    while n < 70 * rate:
        k = capi.feeder_num_ready(n, rate, 1, step, False)
        one = _one_shot(n, rate, step)
        assert capi.feeder_num_ready(n, rate, 2, step, True) == one
        assert prev <= k <= one, (n, prev, k, one)
        assert one - k <= bound, (n, k, one, bound)
        prev = k
        n += 1 if n < 6000 else (53 if n < 4 * rate else 1009)
    assert capi.feeder_num_ready(10 ** 6, rate, 1, 0, False) == 0 and capi.feeder_num_ready(10 ** 6, rate, 9, 1, True) == 0


def test_feed_without_a_device_fails_loudly():
    f = capi.Feeder(2, 1, 48000, capi.SAMPLE_F32, 2)
    if capi.device_count() > 0:                                       # (with one, the same calls simply work)
        f.feed([np.zeros(48000, dtype=np.float32), None])
        f.finish()
        assert f.ready(0) == (capi.feeder_num_ready(48000, 48000, 1, 2, True), 48000, True)
        return
    with pytest.raises(capi.NeedleError) as e:
        f.feed([np.zeros(48000, dtype=np.float32), None])
    assert "no HIP device" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:                        # the failure poisons the feeder
        f.finish()
    assert "no HIP device" in str(e.value)
    assert f.state_bytes() == (0, 0)
