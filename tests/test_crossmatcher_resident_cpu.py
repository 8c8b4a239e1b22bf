"""Resident videos in the cross-matcher, without a GPU: needle_hip_crossmatcher_new_resident, _state_bytes_resident and
_resident through every layer, the argument checks that come before a device is asked for, the loud failure of creation
when there is none, and the state-size arithmetic.  What needs an object is in tests/test_gpu_crossmatcher_resident.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from needle_amd import capi
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["needle_hip_crossmatcher_new_resident", "needle_hip_crossmatcher_state_bytes_resident", "needle_hip_crossmatcher_resident"]
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
        assert re.search(r"ffi::%s\(" % sym, lib_rs), f"{sym} is not used by lib.rs"
    assert protos["needle_hip_crossmatcher_new_resident"] == (
        ["*const u32", "usize", "*const NeedleHipSeq", "usize", "usize", "usize", "*const usize", "*const u32", "u32",
         "*mut *mut NeedleHipCrossMatcher"], "NeedleError")
    assert protos["needle_hip_crossmatcher_state_bytes_resident"] == (["*const NeedleHipSeq", "usize", "usize", "usize", "*const usize"], "usize")
    assert protos["needle_hip_crossmatcher_resident"] == (["*const NeedleHipCrossMatcher", "*mut usize"], "NeedleError")
    for name in ("with_resident", "state_bytes"):
        assert callable(getattr(capi.CrossMatcher, name)), name
    assert isinstance(capi.CrossMatcher.resident, property)
    for name in ("pub fn with_resident(", "pub fn resident(", "pub fn state_bytes_resident("):
        assert name in lib_rs, name


def _new(lens=(10, 20), videos=3, max_items=(100,), min_len=(8,), regions=None, arena=None, offsets=None, out=True, seqs=True, hashes=True):
    """The raw call over resident rows of `lens` hashes packed in an arena of `arena` (default: their sum) hashes.
    Returns (error, handle)."""
    h = C.c_void_p()
    regions = len(max_items) if regions is None else regions
    table = np.zeros((max(len(lens), 1), 2), dtype=np.uint32)
    table[:len(lens), 1] = lens
    table[:len(lens), 0] = np.cumsum([0] + list(lens))[:len(lens)] if offsets is None else offsets
    arena = sum(lens) if arena is None else arena
    store = np.zeros(max(min(arena, 1 << 20), 1), dtype=np.uint32)              # (a refused call never reads it)
    mi = None if max_items is None else (C.c_size_t * max(len(max_items), 1))(*max_items)
    ml = None if min_len is None else (C.c_uint32 * max(len(min_len), 1))(*min_len)
    k = len(lens) // max(regions, 1)
    err = capi.lib().needle_hip_crossmatcher_new_resident(store.ctypes.data if hashes else None, arena, table.ctypes.data if seqs else None, k,
                                                          videos, regions, mi, ml, 10, C.byref(h) if out else None)
    return err, h


def _refused(**kw):
    """InvalidArgument whether or not there is a device: the check comes before it."""
    err, h = _new(**kw)
    assert h.value is None
    return err == INVALID


def test_creation_checks_its_arguments_before_it_asks_for_a_device():
    assert _new(out=False)[0] == NULL
    assert _new(max_items=None, regions=1)[0] == NULL
    assert _new(min_len=None)[0] == NULL
    assert _new(seqs=False)[0] == NULL
    assert _new(hashes=False)[0] == NULL
    for regions in (0, 3):
        assert _refused(lens=(10,) * 6, regions=regions, max_items=(100, 50, 25), min_len=(8, 5, 3)), regions
    for videos in (0, 257, 65536):                                               # N is 1 .. 256 when K >= 1
        assert _refused(videos=videos), videos
    assert _refused(lens=(), videos=1)                                           # ... and 2 .. 256 when K = 0
    assert _refused(lens=(), videos=0) and _refused(lens=(), videos=257)
    for max_items in ((1,), (0,), (2 ** 31,), (2 ** 31 - 15,), (100, 1), (1, 100)):
        assert _refused(lens=(10, 20), max_items=max_items, min_len=(8, 5)[:len(max_items)]), max_items
    for min_len in ((0,), (8, 0), (0, 5)):
        assert _refused(lens=(10, 20), max_items=(100, 50)[:len(min_len)], min_len=min_len), min_len
    # a resident row past the arena, by its length or by its offset; a row that is too long
    assert _refused(lens=(10, 20), arena=29)
    assert _refused(lens=(10, 20), offsets=[0, 11])
    assert _refused(lens=(10, 20), offsets=[2 ** 32 - 1, 0], arena=30)
    assert _refused(lens=(2 ** 31 - 15,), arena=2 ** 31)
    # live problems: (K N + N (N - 1) / 2) x regions <= 65 535
    assert _refused(lens=(2,) * 255, videos=256)                                 # 65 280 + 32 640
    assert _refused(lens=(2,) * 65536, videos=1)                                 # exactly 65 536
    assert _refused(lens=(2,) * (2 * 32768), videos=1, max_items=(100, 50), min_len=(8, 5))   # 32 768 x 2 regions
    assert _refused(lens=(2,) * 2000 * 2, videos=28, max_items=(100, 50), min_len=(8, 5))     # 112 756
    for call in (lambda: capi.CrossMatcher.with_resident([np.zeros(4, np.uint32)], 0, [10], [1], 10),
                 lambda: capi.CrossMatcher.with_resident([np.zeros(4, np.uint32)] * 255, 256, [10], [1], 10),
                 lambda: capi.CrossMatcher.with_resident([np.zeros(4, np.uint32)], 2, [10], [0], 10),
                 lambda: capi.CrossMatcher.with_resident([], 1, [10], [1], 10)):
        with pytest.raises(capi.NeedleError) as e:
            call()
        assert e.value.code == INVALID
    with pytest.raises(ValueError):
        capi.CrossMatcher.with_resident([np.zeros(4, np.uint32)] * 3, 2, [10, 10], [1, 1], 10)   # three rows, two regions


ACCEPTED = [dict(lens=(2,) * 32767, videos=2),                                   # exactly 65 535 live problems
            dict(lens=(2,) * 65535, videos=1),                                   # ... with one arriving video
            dict(lens=(10, 20), videos=1),                                       # N = 1 with K >= 1
            dict(lens=(0, 1, 5), videos=2),                                      # rows of 0 and 1 hashes
            dict(lens=(10, 0, 0, 20), videos=2, max_items=(100, 50), min_len=(8, 5)),
            dict(lens=(), videos=2)]                                             # K = 0: new_regions


def test_creation_without_a_device_fails_loudly():
    """What passes the checks reaches the device: with one the object exists, without one the failure says so."""
    for kw in ACCEPTED:
        err, h = _new(**kw)
        if capi.device_count() > 0:
            assert err == 0 and h.value, kw
            k = C.c_size_t()
            assert capi.lib().needle_hip_crossmatcher_resident(h, C.byref(k)) == 0
            assert k.value == len(kw["lens"]) // len(kw.get("max_items", (1,)))
            capi.lib().needle_hip_crossmatcher_free(h)
        else:
            assert err not in (0, INVALID, NULL) and h.value is None, kw
            assert "no HIP device" in (capi.lib().needle_hip_last_error_message() or b"").decode(), kw
    if capi.device_count() > 0:
        return
    with pytest.raises(capi.NeedleError) as e:
        capi.CrossMatcher.with_resident([np.arange(10, dtype=np.uint32)], 2, [40], [2], 10)
    assert "no HIP device" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:                                   # argument errors come first, device or not
        capi.CrossMatcher.with_resident([np.arange(10, dtype=np.uint32)], 2, [40], [0], 10)
    assert "min_len" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:
        capi.CrossMatcher.with_resident([np.arange(10, dtype=np.uint32)] * 255, 256, [40], [2], 10)
    assert "live problems" in str(e.value)


def test_resident_without_an_object_is_a_null_argument():
    k = C.c_size_t()
    assert capi.lib().needle_hip_crossmatcher_resident(None, C.byref(k)) == NULL


def _formula(lens, videos, max_items):
    regions = len(max_items)
    pairs = videos * (videos - 1) // 2
    w = 2 if all(x < 65536 for x in max_items) and all(x < 65536 for x in lens) else 4
    total = 0
    for r in range(regions):
        s = sum(lens[r::regions])
        total += pairs * 4 * max_items[r] * w + videos * max_items[r] * 4 + videos * 2 * s * w + s * 4
    return total


@pytest.mark.parametrize("lens,videos,max_items", [
    ((5441,) * 1000, 28, (5441,)),                                               # the worked example
    ((10, 20), 1, (100,)), ((10, 20, 30, 40), 3, (100, 50)), ((0, 1, 5), 2, (7,)), ((0, 0, 0, 0), 2, (7, 9)),
    ((65535,), 2, (48,)), ((65536,), 2, (48,)), ((100, 65536), 2, (48, 48)), ((65536, 100), 2, (48, 48)), ((100,), 2, (65536,)),
    ((2,) * 32767, 2, (2,)), ((), 28, (2897, 1443)), ((), 5, (300,))])
def test_state_bytes_resident_is_the_formula(lens, videos, max_items):
    assert capi.CrossMatcher.state_bytes(videos, max_items, lens) == _formula(lens, videos, max_items) > 0


def test_state_bytes_resident_worked_example_width_and_range():
    sb = capi.CrossMatcher.state_bytes
    assert sb(28, (5441,), (5441,) * 1000) == sb(28, 5441, (5441,) * 1000) == 648_218_976
    for videos, max_items in ((28, (2897, 1443)), (5, (300,)), (256, (5441, 2720))):   # K = 0: the regions call
        assert sb(videos, max_items, ()) == sb(videos, max_items) > 0
    # only a RESIDENT row reaches 65 536: every entry of the object widens, the arriving pairs' too
    assert sb(3, (48,), (65535,)) == 3 * 4 * 48 * 2 + 3 * 48 * 4 + 3 * 2 * 65535 * 2 + 65535 * 4
    assert sb(3, (48,), (65536,)) == 3 * 4 * 48 * 4 + 3 * 48 * 4 + 3 * 2 * 65536 * 4 + 65536 * 4
    assert sb(3, (48, 48), (10, 65536)) - sb(3, (48, 48), (10, 65535)) == 3 * 4 * 96 * 2 + 3 * 2 * (10 * 2 + 65536 * 4 - 65535 * 2) + 4
    # empty resident rows add nothing; a resident video costs nothing per arriving pair
    assert sb(3, (48,), (0, 0, 0)) == sb(3, (48,), ()) == sb(3, 48)
    assert sb(3, (48,), (0, 7, 0)) - sb(3, 48) == 3 * 2 * 7 * 2 + 7 * 4
    # out of range: no such matcher
    for videos, max_items, lens in ((0, (10,), (5,)), (257, (10,), (5,)), (1, (10,), ()), (2, (1,), (5,)), (2, (10,), (2 ** 31 - 15,)),
                                    (256, (10,), (2,) * 255), (1, (10,), (2,) * 65536), (2, (10, 10, 10), (5,) * 3), (2, (), ())):
        assert sb(videos, max_items, lens) == 0, (videos, max_items, len(lens))
    assert capi.lib().needle_hip_crossmatcher_state_bytes_resident(None, 0, 4, 2, None) == 0
    assert capi.lib().needle_hip_crossmatcher_state_bytes_resident(None, 3, 4, 1, (C.c_size_t * 1)(10)) == 0
