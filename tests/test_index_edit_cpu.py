"""CPU tests of the incremental index's removal and replacement (needle_hip_index_remove / _replace / _store_sizes,
include/needle_hip.h "Incremental index"): the symbols, argument validation, and an empty index that stays empty."""
import ctypes as C
import os

import pytest

from needle_amd import capi

OK, NULL_ARGUMENT, INVALID_ARGUMENT = 0, capi.ERROR_NAMES.index("NullArgument"), capi.ERROR_NAMES.index("InvalidArgument")
EDIT_SYMBOLS = ["needle_hip_index_remove", "needle_hip_index_replace", "needle_hip_index_store_sizes"]


def _frame_hashes(count=2):
    return [capi.FrameHashes.new([(i * 7 + k, 2_600_000_000 + i * 246_000_000) for i in range(100)], [], 300_000_012)
            for k in range(count)]


def test_edit_symbols_are_declared_exported_and_listed():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "needle_hip.h")) as f:
        header = f.read()
    for name in EDIT_SYMBOLS:
        assert name + "(" in header
        assert name in capi.NEEDLE_HIP_H_SYMBOLS
        assert hasattr(capi.lib(), name)


def test_edit_validates_its_arguments():
    L = capi.lib()
    index = capi.Index(capi.Comparator(["a.mkv", "b.mkv"]))
    h = index._h
    pos = (C.c_size_t * 2)(0, 1)
    fhs = _frame_hashes()
    ptrs = (C.c_void_p * 2)(*[f._h for f in fhs])
    sizes = (C.c_uint64 * 4)()
    # NULL pointers
    assert L.needle_hip_index_remove(None, pos, C.c_size_t(1)) == NULL_ARGUMENT
    assert L.needle_hip_index_remove(h, None, C.c_size_t(1)) == NULL_ARGUMENT
    assert L.needle_hip_index_replace(None, pos, ptrs, C.c_size_t(1)) == NULL_ARGUMENT
    assert L.needle_hip_index_replace(h, None, ptrs, C.c_size_t(1)) == NULL_ARGUMENT
    assert L.needle_hip_index_replace(h, pos, None, C.c_size_t(1)) == NULL_ARGUMENT
    assert L.needle_hip_index_store_sizes(None, sizes) == NULL_ARGUMENT
    assert L.needle_hip_index_store_sizes(h, None) == NULL_ARGUMENT
    # k == 0
    assert L.needle_hip_index_remove(h, pos, C.c_size_t(0)) == INVALID_ARGUMENT
    assert L.needle_hip_index_replace(h, pos, ptrs, C.c_size_t(0)) == INVALID_ARGUMENT
    # positions out of range (the index is empty: every position is)
    assert L.needle_hip_index_remove(h, pos, C.c_size_t(1)) == INVALID_ARGUMENT
    assert L.needle_hip_index_replace(h, pos, ptrs, C.c_size_t(2)) == INVALID_ARGUMENT
    far = (C.c_size_t * 1)(2 ** 40)
    assert L.needle_hip_index_remove(h, far, C.c_size_t(1)) == INVALID_ARGUMENT
    # a NULL FrameHashes among the replacements
    holes = (C.c_void_p * 2)(fhs[0]._h, None)
    assert L.needle_hip_index_replace(h, pos, holes, C.c_size_t(2)) == NULL_ARGUMENT
    for bad in ([], [0], [3, 1]):
        with pytest.raises(capi.NeedleError) as e:
            index.remove(bad)
        assert e.value.name == "InvalidArgument"
    with pytest.raises(capi.NeedleError) as e:
        index.replace([0], fhs[:1])
    assert e.value.name == "InvalidArgument"
    with pytest.raises(ValueError):
        index.replace([0, 1], fhs[:1])
    assert len(index) == 0 and index.results() == [] and index.pairs_searched() == (0, 0)


def test_repeated_positions_are_refused_before_any_device_work():
    """Positions are checked on the host: [0, 0] is refused on any index (on an empty one it is also out of range; a
    filled index's repeated positions: tests/test_gpu_index_edit.py), and store_sizes of an empty index is all zeros."""
    L = capi.lib()
    index = capi.Index(capi.Comparator(["a.mkv", "b.mkv"]))
    twice = (C.c_size_t * 2)(0, 0)
    assert L.needle_hip_index_remove(index._h, twice, C.c_size_t(2)) == INVALID_ARGUMENT
    fhs = _frame_hashes()
    ptrs = (C.c_void_p * 2)(*[f._h for f in fhs])
    assert L.needle_hip_index_replace(index._h, twice, ptrs, C.c_size_t(2)) == INVALID_ARGUMENT
    assert index.store_sizes() == (0, 0, 0, 0)


def test_edit_of_an_empty_index_fails_cleanly_without_a_gpu(has_gpu):
    """No CPU fallback and nothing to edit: remove and replace report InvalidArgument, the index stays empty and
    store_sizes is all zeros (it needs no device when the store is empty)."""
    if has_gpu:
        pytest.skip("a GPU is present; covered by tests/test_gpu_index_edit.py")
    index = capi.Index(capi.Comparator(["a.mkv", "b.mkv"]))
    with pytest.raises(capi.NeedleError) as e:
        index.add(_frame_hashes(2))
    assert e.value.name == "Unknown" and "no HIP device" in str(e.value)
    for call in (lambda: index.remove([0]), lambda: index.replace([0], _frame_hashes(1))):
        with pytest.raises(capi.NeedleError) as e:
            call()
        assert e.value.name == "InvalidArgument"
    assert len(index) == 0 and index.results() == [] and index.pairs_searched() == (0, 0)
    assert index.store_sizes() == (0, 0, 0, 0)
