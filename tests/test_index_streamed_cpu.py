"""A streamed season into an index of any size, without a GPU: needle_hip_index_matcher_new and
needle_hip_index_add_streamed through every layer, their argument checks (which come before a device is asked for), and
the cross-matcher's limit, which stays where it was.  What needs an object is in tests/test_gpu_index_streamed.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from needle_amd import capi
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["needle_hip_index_matcher_new", "needle_hip_index_add_streamed"]
INVALID, NULL = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("NullArgument")


def test_symbols_in_every_layer():
    header = R.strip_comments(open(os.path.join(ROOT, "include", "needle_hip.h")).read())
    lib_rs = open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")).read()
    protos = R.c_prototypes()
    fns, _, _ = R.rust_declarations()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(capi.lib(), sym) and sym in capi.NEEDLE_HIP_H_SYMBOLS, sym
        assert fns[sym] == protos[sym], (sym, fns[sym], protos[sym])
        assert re.search(r"ffi::%s\(" % sym, lib_rs), f"{sym} is not used by lib.rs"
    assert protos["needle_hip_index_matcher_new"] == (["*mut NeedleHipIndex", "usize", "*mut *mut NeedleHipMatcher"], "NeedleError")
    assert protos["needle_hip_index_add_streamed"] == (
        ["*mut NeedleHipIndex", "*mut NeedleHipMatcher", "*mut NeedleHipCrossMatcher", "*const *const FrameHashes", "usize"], "NeedleError")
    assert callable(capi.Index.matcher) and callable(capi.Index.add_streamed)
    assert "pub fn matcher(" in lib_rs and "pub fn add_streamed(" in lib_rs


def _index(endings=False):
    return capi.Index(capi.Comparator(["a.wav", "b.wav"], include_endings=endings, min_opening_duration=10))


def test_a_matcher_from_an_empty_index_is_refused_and_says_where_to_go():
    """An empty index has nothing resident; the refusal needs no device and names the index's cross-matcher."""
    for endings in (False, True):
        index = _index(endings)
        for videos in (1, 28, 65535, 0):
            with pytest.raises(capi.NeedleError) as e:
                index.matcher(videos)
            assert e.value.code == INVALID and "needle_hip_index_crossmatcher_new" in str(e.value), str(e.value)
        assert len(index) == 0 and index.pairs_searched() == (0, 0)


def test_null_arguments():
    L = capi.lib()
    index = _index()
    h = C.c_void_p()
    assert L.needle_hip_index_matcher_new(None, 2, C.byref(h)) == NULL
    assert L.needle_hip_index_matcher_new(index._h, 2, None) == NULL
    fh = capi.FrameHashes.new([(1, 0), (2, 246_000_000)], [], 300_000_000)
    ptrs = (C.c_void_p * 1)(fh._h)
    fake = C.c_void_p(1)                                                         # (never dereferenced: a NULL comes first)
    assert L.needle_hip_index_add_streamed(None, fake, None, ptrs, 1) == NULL
    assert L.needle_hip_index_add_streamed(index._h, None, None, ptrs, 1) == NULL
    assert len(index) == 0


def test_the_cross_matchers_limit_stays_where_it_was():
    """129 resident and 256 arriving videos, two regions: (129 x 256 + 256 x 255 / 2) x 2 = 131 328 live problems.  Refused
    in the words it always was; the cross-matcher of the 256 arriving videos alone, 65 280, passes the checks."""
    rows = [np.zeros(2, np.uint32)] * (129 * 2)
    with pytest.raises(capi.NeedleError) as e:
        capi.CrossMatcher.with_resident(rows, 256, [40, 40], [2, 2], 10)
    assert e.value.code == INVALID and "live problems" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:                                   # 2 000 + 28 x 2 regions: the header's example
        capi.CrossMatcher.with_resident([np.zeros(2, np.uint32)] * 4000, 28, [40, 40], [2, 2], 10)
    assert e.value.code == INVALID and "live problems" in str(e.value)
    if capi.device_count() == 0:
        with pytest.raises(capi.NeedleError) as e:
            capi.CrossMatcher.with_regions(256, [40, 40], [2, 2], 10)
        assert e.value.code != INVALID and "no HIP device" in str(e.value)
        with pytest.raises(capi.NeedleError) as e:                               # ... and so does the one an empty index makes
            _index(True).crossmatcher(256, [40, 40], [2, 2])
        assert e.value.code != INVALID and "no HIP device" in str(e.value)
