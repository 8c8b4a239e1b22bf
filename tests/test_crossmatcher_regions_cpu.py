"""The two-region cross-matcher's boundary without a GPU: needle_hip_crossmatcher_new_regions, _state_bytes_regions and
_shape through every layer, the argument checks that come before a device is asked for, the loud failure of creation when
there is none, and the state-size arithmetic (one entry width for the whole object).  What needs an object is in
tests/test_gpu_crossmatcher_regions.py."""
import ctypes as C
import os
import re

import pytest

from needle_amd import capi
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["needle_hip_crossmatcher_new_regions", "needle_hip_crossmatcher_state_bytes_regions", "needle_hip_crossmatcher_shape"]
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
    assert protos["needle_hip_crossmatcher_new_regions"] == (["usize", "usize", "*const usize", "*const u32", "u32",
                                                              "*mut *mut NeedleHipCrossMatcher"], "NeedleError")
    assert protos["needle_hip_crossmatcher_state_bytes_regions"] == (["usize", "usize", "*const usize"], "usize")
    assert protos["needle_hip_crossmatcher_shape"] == (["*const NeedleHipCrossMatcher", "*mut usize", "*mut usize"], "NeedleError")
    for name in ("with_regions", "shape", "state_bytes"):
        assert callable(getattr(capi.CrossMatcher, name)), name


def _new(videos=4, max_items=(100, 50), min_len=(8, 5), threshold=10, regions=None, out=True):
    """The raw call; max_items / min_len None: a NULL array.  Returns (error, handle)."""
    h = C.c_void_p()
    regions = len(max_items) if regions is None else regions
    mi = None if max_items is None else (C.c_size_t * max(len(max_items), 1))(*max_items)
    ml = None if min_len is None else (C.c_uint32 * max(len(min_len), 1))(*min_len)
    return capi.lib().needle_hip_crossmatcher_new_regions(videos, regions, mi, ml, threshold, C.byref(h) if out else None), h


def test_creation_checks_its_arguments_before_it_asks_for_a_device():
    assert _new(out=False)[0] == NULL
    assert _new(max_items=None, regions=2)[0] == NULL
    assert _new(min_len=None)[0] == NULL
    for regions in (0, 3):
        assert _new(regions=regions, max_items=(100, 50, 25), min_len=(8, 5, 3))[0] == INVALID, regions
    for videos in (0, 1, 257, 65536):
        assert _new(videos=videos)[0] == INVALID, videos
        assert _new(videos=videos, max_items=(100,), min_len=(8,))[0] == INVALID, videos
    for max_items in ((1, 50), (100, 1), (0, 50), (100, 0), (2 ** 31, 50), (100, 2 ** 31), (1,)):
        assert _new(max_items=max_items, min_len=(8, 5)[:len(max_items)])[0] == INVALID, max_items
    for min_len in ((0, 5), (8, 0), (0,)):
        assert _new(max_items=(100, 50)[:len(min_len)], min_len=min_len)[0] == INVALID, min_len
    for call in (lambda: capi.CrossMatcher.with_regions(4, (100, 50), (8, 0), 10), lambda: capi.CrossMatcher.with_regions(4, (100, 1), (8, 5), 10),
                 lambda: capi.CrossMatcher.with_regions(300, (100, 50), (8, 5), 10), lambda: capi.CrossMatcher.with_regions(4, (9, 9, 9), (1, 1, 1), 10),
                 lambda: capi.CrossMatcher.with_regions(4, (), (), 10)):
        with pytest.raises(capi.NeedleError) as e:
            call()
        assert e.value.code == INVALID


def test_shape_without_an_object_is_a_null_argument():
    videos, regions = C.c_size_t(), C.c_size_t()
    assert capi.lib().needle_hip_crossmatcher_shape(None, C.byref(videos), C.byref(regions)) == NULL


def test_creation_without_a_device_fails_loudly():
    if capi.device_count() > 0:                                       # (with one, the same call simply works)
        m = capi.CrossMatcher.with_regions(3, (40, 20), (2, 2), 10)
        assert m.shape() == (3, 2) and m.lanes == 6 and m.ready() == (0, False) and m.lane(5) == (0, False)
        assert capi.CrossMatcher(3, 40, 2, 10).shape() == (3, 1)
        return
    for regions in (1, 2):
        with pytest.raises(capi.NeedleError) as e:
            capi.CrossMatcher.with_regions(3, (40, 20)[:regions], (2, 2)[:regions], 10)
        assert "no HIP device" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:                        # argument errors come first, device or not
        capi.CrossMatcher.with_regions(3, (40, 20), (2, 0), 10)
    assert "min_len" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:
        capi.CrossMatcher.with_regions(3, (40, 20, 10), (2, 2, 2), 10)
    assert "regions" in str(e.value)


def _formula(videos, max_items):
    pairs = videos * (videos - 1) // 2
    w = 2 if all(x < 65536 for x in max_items) else 4
    return sum(pairs * 2 * 2 * x * w + videos * x * 4 for x in max_items)


@pytest.mark.parametrize("videos,max_items", [(2, (2, 2)), (28, (2897, 1443)), (256, (5441, 2720)), (3, (65535, 65535)), (3, (65536, 100)),
                                              (3, (100, 65536)), (3, (48, 65540)), (5, (300,)), (3, (65536,))])
def test_state_bytes_regions_is_the_formula(videos, max_items):
    assert capi.CrossMatcher.state_bytes(videos, max_items) == _formula(videos, max_items)


def test_state_bytes_regions_width_range_and_the_single_region_call():
    sb = capi.CrossMatcher.state_bytes
    assert sb(2, (2, 2)) == 2 * (2 * 2 * 2 * 2 + 2 * 2 * 4) == 64
    for videos, x in ((2, 2), (28, 5441), (3, 65535), (3, 65536), (256, 100)):   # regions = 1: the single-region call
        assert sb(videos, (x,)) == sb(videos, x) > 0
    # one width for the whole object: it switches at 65 536 on the larger region, and the smaller region's entries widen too
    assert sb(3, (65535, 100)) == 3 * 4 * (65535 + 100) * 2 + 3 * (65535 + 100) * 4
    assert sb(3, (65536, 100)) == 3 * 4 * (65536 + 100) * 4 + 3 * (65536 + 100) * 4
    assert sb(3, (100, 65535)) == sb(3, (65535, 100)) and sb(3, (100, 65536)) == sb(3, (65536, 100))
    assert sb(3, (65536, 100)) != sb(3, 65536) + sb(3, 100)                     # (region 1 alone would be 16-bit)
    assert sb(3, (65535, 100)) == sb(3, 65535) + sb(3, 100)
    for videos, max_items in ((1, (10, 10)), (257, (10, 10)), (4, (1, 10)), (4, (10, 1)), (4, (10, 2 ** 31)), (4, ()), (4, (10, 10, 10))):
        assert sb(videos, max_items) == 0, (videos, max_items)                   # out of range: no such matcher
    assert capi.lib().needle_hip_crossmatcher_state_bytes_regions(4, 2, None) == 0
