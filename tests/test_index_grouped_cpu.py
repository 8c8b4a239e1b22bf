"""CPU tests of the grouped incremental index (needle_hip_index_new_grouped / _add_grouped / _groups, include/needle_hip.h
"A grouped index"): the symbols, argument validation, and the refusals that are decided before the store is touched -- an
add without labels on a grouped index, labels on a plain one, the four streamed routes on a grouped one."""
import ctypes as C
import os
import re

import pytest

from needle_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL_ARGUMENT, INVALID_ARGUMENT = 0, capi.ERROR_NAMES.index("NullArgument"), capi.ERROR_NAMES.index("InvalidArgument")
GROUPED_SYMBOLS = ["needle_hip_index_new_grouped", "needle_hip_index_add_grouped", "needle_hip_index_groups"]


def _frame_hashes(count=2):
    return [capi.FrameHashes.new([(i * 7 + k, 2_600_000_000 + i * 246_000_000) for i in range(100)], [], 300_000_012)
            for k in range(count)]


def _comparator():
    return capi.Comparator(["a.mkv", "b.mkv"])


def test_grouped_symbols_are_declared_exported_bound_and_named_in_rust():
    with open(os.path.join(ROOT, "include", "needle_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "rust", "needle-hip", "src", "ffi.rs")) as f:
        ffi = f.read()
    with open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")) as f:
        wrapper = f.read()
    for name in GROUPED_SYMBOLS:
        assert name + "(" in header
        assert name in capi.NEEDLE_HIP_H_SYMBOLS
        assert hasattr(capi.lib(), name)
        assert getattr(capi.lib(), name).argtypes is not None, "bound with its argument types"
        assert re.search(r"pub fn %s\(" % name, ffi) and "ffi::%s(" % name in wrapper
    assert "const uint32_t *groups" in header[header.index("needle_hip_index_add_grouped("):][:200]


def test_grouped_calls_validate_their_arguments():
    L = capi.lib()
    cmp = _comparator()
    index = capi.Index(cmp, grouped=True)
    assert index.grouped and len(index) == 0 and index.groups() == []
    h = index._h
    fhs = _frame_hashes()
    ptrs = (C.c_void_p * 2)(*[f._h for f in fhs])
    labels = (C.c_uint32 * 2)(7, 7)
    out = C.c_void_p()
    # NULL pointers
    assert L.needle_hip_index_new_grouped(None, C.byref(out)) == NULL_ARGUMENT
    assert L.needle_hip_index_new_grouped(cmp.handle(), None) == NULL_ARGUMENT
    assert L.needle_hip_index_add_grouped(None, ptrs, labels, 2) == NULL_ARGUMENT
    assert L.needle_hip_index_add_grouped(h, None, labels, 2) == NULL_ARGUMENT
    assert L.needle_hip_index_add_grouped(h, ptrs, None, 2) == NULL_ARGUMENT
    assert L.needle_hip_index_groups(None, labels, 2) == NULL_ARGUMENT
    # k == 0, before the pointers are looked at
    assert L.needle_hip_index_add_grouped(h, ptrs, labels, 0) == INVALID_ARGUMENT
    assert L.needle_hip_index_add_grouped(h, None, None, 0) == INVALID_ARGUMENT
    # a NULL FrameHashes among the videos
    holes = (C.c_void_p * 2)(fhs[0]._h, None)
    assert L.needle_hip_index_add_grouped(h, holes, labels, 2) == NULL_ARGUMENT
    # an empty grouped index has no labels: any buffer will do, NULL too
    assert L.needle_hip_index_groups(h, None, 0) == OK
    assert L.needle_hip_index_groups(h, labels, 2) == OK
    with pytest.raises(ValueError):
        index.add(fhs, groups=[1])
    assert len(index) == 0 and index.results() == [] and index.pairs_searched() == (0, 0) and index.store_sizes() == (0, 0, 0, 0)


def test_the_wrong_kind_of_index_is_refused_before_the_store_is_touched():
    """Decided on the host: these answer the same with or without a device, and leave both indexes empty."""
    L = capi.lib()
    cmp = _comparator()
    grouped, plain = capi.Index(cmp, grouped=True), capi.Index(cmp)
    fhs = _frame_hashes()
    ptrs = (C.c_void_p * 2)(*[f._h for f in fhs])
    labels = (C.c_uint32 * 2)(1, 1)
    # add without labels on a grouped index; labels on a plain one; the labels of a plain one
    with pytest.raises(capi.NeedleError) as e:
        grouped.add(fhs)
    assert e.value.name == "InvalidArgument" and "grouped index takes a label per video" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:
        plain.add(fhs, groups=[1, 1])
    assert e.value.name == "InvalidArgument" and "not a grouped index" in str(e.value)
    assert L.needle_hip_index_add_grouped(plain._h, ptrs, labels, 2) == INVALID_ARGUMENT
    assert L.needle_hip_index_groups(plain._h, labels, 2) == INVALID_ARGUMENT
    with pytest.raises(capi.NeedleError) as e:
        plain.groups()
    assert e.value.name == "InvalidArgument" and "not a grouped index" in str(e.value)
    # the four streamed routes on a grouped index (NULL matchers: the kind of index is looked at first where the C ABI lets it be)
    out = C.c_void_p()
    items, min_len = (C.c_size_t * 1)(100), (C.c_uint32 * 1)(21)
    assert L.needle_hip_index_crossmatcher_new(grouped._h, 2, items, min_len, C.byref(out)) == INVALID_ARGUMENT
    assert b"grouped index has no streamed routes" in L.needle_hip_last_error_message()
    assert L.needle_hip_index_matcher_new(grouped._h, 2, C.byref(out)) == INVALID_ARGUMENT
    assert b"grouped index has no streamed routes" in L.needle_hip_last_error_message()
    assert out.value is None
    for ix in (grouped, plain):
        assert len(ix) == 0 and ix.results() == [] and ix.pairs_searched() == (0, 0) and ix.store_sizes() == (0, 0, 0, 0)
    assert grouped.groups() == []


def test_a_grouped_add_fails_cleanly_without_a_gpu(has_gpu):
    """No CPU fallback: with labels and no device the add reports the missing device and the index stays empty."""
    if has_gpu:
        pytest.skip("a GPU is present; covered by tests/test_gpu_index_grouped.py")
    index = capi.Index(_comparator(), grouped=True)
    with pytest.raises(capi.NeedleError) as e:
        index.add(_frame_hashes(2), groups=[3, 3])
    assert e.value.name == "Unknown" and "no HIP device" in str(e.value)
    assert len(index) == 0 and index.groups() == [] and index.pairs_searched() == (0, 0)
