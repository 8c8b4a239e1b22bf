"""The streaming all-pairs comparator's boundary without a GPU: the ten needle_hip_crossmatcher_* symbols through every
layer, the argument errors that are checked before any device work, the loud failure of creation when there is no device
(state and histories are allocated at creation, so a cross-matcher cannot exist without one: the errors that need an
object are in tests/test_gpu_crossmatcher.py), and the state-size arithmetic."""
import ctypes as C
import os
import re

import pytest

from needle_amd import capi
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["needle_hip_crossmatcher_new", "needle_hip_crossmatcher_free", "needle_hip_crossmatcher_feed",
           "needle_hip_crossmatcher_feed_from_feeder", "needle_hip_crossmatcher_finish", "needle_hip_crossmatcher_ready",
           "needle_hip_crossmatcher_lane", "needle_hip_crossmatcher_runs", "needle_hip_crossmatcher_stats",
           "needle_hip_crossmatcher_state_bytes"]
INVALID, NULL = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("NullArgument")


def test_symbols_in_every_layer():
    header = R.strip_comments(open(os.path.join(ROOT, "include", "needle_hip.h")).read())
    lib_rs = open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")).read()
    makefile = open(os.path.join(ROOT, "needle_amd", "csrc", "Makefile")).read()
    protos = R.c_prototypes()
    fns, _, _ = R.rust_declarations()
    L = capi.lib()
    assert len(SYMBOLS) == 10
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(L, sym), sym
        assert sym in capi.NEEDLE_HIP_H_SYMBOLS, sym
        assert sym in fns, f"{sym} is not declared in ffi.rs"
        assert fns[sym] == protos[sym], (sym, fns[sym], protos[sym])
        assert "ffi::%s(" % sym in lib_rs, f"{sym} is not used by lib.rs"
    assert "typedef struct NeedleHipCrossMatcher NeedleHipCrossMatcher;" in header
    assert hasattr(capi, "CrossMatcher")
    assert re.search(r"^HIP_SRC\s*=.*\bcrossmatch\.hip\b", makefile, re.M) and re.search(r"^HDR\s*=.*\bcrossmatch\.h\b", makefile, re.M)
    assert os.path.exists(os.path.join(ROOT, "needle_amd", "csrc", "crossmatch.h"))


def _new(lanes=4, max_items=100, min_len=8, threshold=10, out=True):
    h = C.c_void_p()
    return capi.lib().needle_hip_crossmatcher_new(lanes, max_items, min_len, threshold, C.byref(h) if out else None), h


def test_creation_checks_its_arguments_before_it_asks_for_a_device():
    assert _new(out=False)[0] == NULL
    for lanes in (0, 1, 257, 65536):
        assert _new(lanes=lanes)[0] == INVALID, lanes
    for max_items in (0, 1, 2 ** 31):
        assert _new(max_items=max_items)[0] == INVALID, max_items
    assert _new(min_len=0)[0] == INVALID


def test_calls_without_an_object_are_null_arguments():
    L = capi.lib()
    ptrs, lens = (C.c_void_p * 2)(), (C.c_size_t * 2)(0, 0)
    runs, fed, fin = C.c_size_t(), C.c_uint64(), C.c_bool()
    assert L.needle_hip_crossmatcher_feed(None, ptrs, lens) == NULL
    assert L.needle_hip_crossmatcher_feed_from_feeder(None, None) == NULL
    assert L.needle_hip_crossmatcher_finish(None, None, 0) == NULL
    assert L.needle_hip_crossmatcher_ready(None, C.byref(runs), C.byref(fin)) == NULL
    assert L.needle_hip_crossmatcher_lane(None, 0, C.byref(fed), C.byref(fin)) == NULL
    assert L.needle_hip_crossmatcher_runs(None, 0, 0, None) == NULL
    assert L.needle_hip_crossmatcher_stats(None, (C.c_uint64 * 4)()) == NULL
    L.needle_hip_crossmatcher_free(None)
    f = C.c_void_p()
    assert L.needle_hip_feeder_new(2, 1, 11025, capi.SAMPLE_S16, 1, C.byref(f)) == 0
    assert L.needle_hip_crossmatcher_feed_from_feeder(None, f) == NULL
    L.needle_hip_feeder_free(f)


def test_creation_without_a_device_fails_loudly():
    if capi.device_count() > 0:                                       # (with one, the same call simply works)
        m = capi.CrossMatcher(3, 40, 2, 10)
        assert m.ready() == (0, False) and m.lane(2) == (0, False) and m.stats()[:3] == (0, 0, 0)
        return
    with pytest.raises(capi.NeedleError) as e:
        capi.CrossMatcher(3, 40, 2, 10)
    assert "no HIP device" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:                        # argument errors come first, device or not
        capi.CrossMatcher(3, 40, 0, 10)
    assert "min_len" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:
        capi.CrossMatcher(300, 40, 2, 10)
    assert "lanes" in str(e.value)


def _formula(lanes, max_items):
    pairs = lanes * (lanes - 1) // 2
    return pairs * 2 * 2 * max_items * (2 if max_items < 65536 else 4) + lanes * max_items * 4


@pytest.mark.parametrize("lanes,max_items", [(2, 2), (28, 5441), (3, 65535), (3, 65536)])
def test_state_bytes_is_the_formula(lanes, max_items):
    assert capi.CrossMatcher.state_bytes(lanes, max_items) == _formula(lanes, max_items)


def test_state_bytes_entry_width_and_range():
    sb = capi.CrossMatcher.state_bytes
    assert sb(2, 2) == 2 * 2 * 2 * 2 + 2 * 2 * 4 == 32
    assert sb(28, 5441) == 378 * 4 * 5441 * 2 + 28 * 5441 * 4                   # 16.5 MB + 0.6 MB
    assert sb(3, 65535) == 3 * 4 * 65535 * 2 + 3 * 65535 * 4                     # 16-bit entries below 65 536 items ...
    assert sb(3, 65536) == 3 * 4 * 65536 * 4 + 3 * 65536 * 4                     # ... 32-bit from there on
    assert sb(3, 65536) - sb(3, 65535) > 3 * 4 * 65535 * 2
    assert sb(1, 10) == 0 and sb(257, 10) == 0 and sb(4, 1) == 0               # out of range: no such matcher
