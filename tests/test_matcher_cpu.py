"""The streaming comparator's boundary without a GPU: the ten needle_hip_matcher_* symbols through every layer, the
argument errors that are checked before any device work, and the loud failure of creation when there is no device (the
sources are uploaded at creation, so a matcher cannot exist without one: the errors that need an object -- a lane out of
range, items for a finished lane, unequal lane counts -- are in tests/test_gpu_matcher.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from needle_amd import capi
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["needle_hip_matcher_new", "needle_hip_matcher_free", "needle_hip_matcher_feed", "needle_hip_matcher_feed_from_feeder",
           "needle_hip_matcher_finish", "needle_hip_matcher_reset", "needle_hip_matcher_ready", "needle_hip_matcher_runs",
           "needle_hip_matcher_open", "needle_hip_matcher_stats"]
INVALID, NULL = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("NullArgument")


def test_symbols_in_every_layer():
    header = R.strip_comments(open(os.path.join(ROOT, "include", "needle_hip.h")).read())
    lib_rs = open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")).read()
    protos = R.c_prototypes()
    fns, structs, _ = R.rust_declarations()
    L = capi.lib()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(L, sym), sym
        assert sym in capi.NEEDLE_HIP_H_SYMBOLS, sym
        assert sym in fns, f"{sym} is not declared in ffi.rs"
        assert fns[sym] == protos[sym], (sym, fns[sym], protos[sym])
        assert "ffi::%s(" % sym in lib_rs, f"{sym} is not used by lib.rs"
    assert "typedef struct NeedleHipMatcher NeedleHipMatcher;" in header
    assert structs["NeedleHipSeq"] == [("offset", "u32"), ("len", "u32")]
    assert hasattr(capi, "Matcher")


def _new(hashes=8, seqs=((0, 8),), min_len=(1,), num_sources=None, lanes=1, threshold=10, out=True, null=()):
    arena = np.arange(hashes, dtype=np.uint32)
    cs = (capi.Seq * max(len(seqs), 1))(*[capi.Seq(o, n) for o, n in seqs])
    ml = (C.c_uint32 * max(len(min_len), 1))(*min_len)
    h = C.c_void_p()
    code = capi.lib().needle_hip_matcher_new(None if "hashes" in null else arena.ctypes.data, arena.size,
                                             None if "sources" in null else C.cast(cs, C.c_void_p),
                                             None if "min_len" in null else C.cast(ml, C.c_void_p),
                                             len(seqs) if num_sources is None else num_sources, lanes, threshold,
                                             C.byref(h) if out else None)
    return code, h


def test_creation_checks_its_arguments_before_it_asks_for_a_device():
    assert _new(out=False)[0] == NULL
    for which in ("hashes", "sources", "min_len"):
        assert _new(null=(which,))[0] == NULL, which
    assert _new(lanes=0)[0] == INVALID
    assert _new(lanes=65536)[0] == INVALID
    assert _new(num_sources=0)[0] == INVALID
    assert _new(min_len=(0,))[0] == INVALID
    assert _new(seqs=((0, 4), (4, 4)), min_len=(3, 0))[0] == INVALID                    # any source's, not only the first
    assert _new(seqs=((1, 8),))[0] == INVALID and _new(seqs=((0, 9),))[0] == INVALID    # a source outside `hashes`
    assert _new(seqs=((0, 8), (0xFFFFFFFF, 2)), min_len=(1, 1))[0] == INVALID           # offset + len does not wrap
    assert _new(hashes=0, seqs=((0, 1),), null=("hashes",))[0] == INVALID               # no hashes at all: outside, not NULL


def test_calls_without_an_object_are_null_arguments():
    L = capi.lib()
    ptrs, lens = (C.c_void_p * 1)(), (C.c_size_t * 1)(0)
    runs, fed, fin = C.c_size_t(), C.c_uint64(), C.c_bool()
    out, n = C.c_void_p(), C.c_size_t()
    assert L.needle_hip_matcher_feed(None, ptrs, lens) == NULL
    assert L.needle_hip_matcher_feed_from_feeder(None, None) == NULL
    assert L.needle_hip_matcher_finish(None, None, 0) == NULL and L.needle_hip_matcher_reset(None, None, 0) == NULL
    assert L.needle_hip_matcher_ready(None, 0, C.byref(runs), C.byref(fed), C.byref(fin)) == NULL
    assert L.needle_hip_matcher_runs(None, 0, 0, 0, None) == NULL
    assert L.needle_hip_matcher_open(None, 0, C.byref(out), C.byref(n)) == NULL
    assert L.needle_hip_matcher_stats(None, (C.c_uint64 * 4)()) == NULL
    L.needle_hip_matcher_free(None)
    f = C.c_void_p()
    assert L.needle_hip_feeder_new(1, 1, 11025, capi.SAMPLE_S16, 1, C.byref(f)) == 0
    assert L.needle_hip_matcher_feed_from_feeder(None, f) == NULL
    L.needle_hip_feeder_free(f)


def test_creation_without_a_device_fails_loudly():
    src = [np.arange(40, dtype=np.uint32), np.arange(3, dtype=np.uint32)]
    if capi.device_count() > 0:                                       # (with one, the same call simply works)
        m = capi.Matcher(src, [2, 1], 2, 10)
        assert m.ready(1) == (0, 0, False) and m.stats()[:3] == (0, 0, 0)
        return
    with pytest.raises(capi.NeedleError) as e:
        capi.Matcher(src, [2, 1], 2, 10)
    assert "no HIP device" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:                        # argument errors come first, device or not
        capi.Matcher(src, [2, 0], 2, 10)
    assert "min_len" in str(e.value)
