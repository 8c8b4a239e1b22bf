"""CPU tests of the incremental index's C ABI (needle_hip_index_*, include/needle_hip.h "Incremental index"): argument
validation, and an add that fails cleanly, leaving the index untouched, when there is no HIP device."""
import ctypes as C

import pytest

from needle_amd import capi

OK, NULL_ARGUMENT, INVALID_ARGUMENT = 0, capi.ERROR_NAMES.index("NullArgument"), capi.ERROR_NAMES.index("InvalidArgument")


def _frame_hashes(count=2):
    return [capi.FrameHashes.new([(i * 7 + k, 2_600_000_000 + i * 246_000_000) for i in range(100)], [], 300_000_012)
            for k in range(count)]


def test_index_symbols_are_listed():
    for name in ["needle_hip_index_new", "needle_hip_index_free", "needle_hip_index_len", "needle_hip_index_add",
                 "needle_hip_index_results", "needle_hip_index_pairs_searched"]:
        assert name in capi.NEEDLE_HIP_H_SYMBOLS
        assert hasattr(capi.lib(), name)


def test_index_validates_its_arguments():
    L = capi.lib()
    out = C.c_void_p()
    assert L.needle_hip_index_new(None, C.byref(out)) == NULL_ARGUMENT
    cmp = capi.Comparator(["a.mkv", "b.mkv"])
    assert L.needle_hip_index_new(cmp.handle(), None) == NULL_ARGUMENT
    L.needle_hip_index_free(None)                                   # free(NULL) is a no-op
    assert L.needle_hip_index_len(None) == 0
    fhs = _frame_hashes()
    ptrs = (C.c_void_p * 2)(*[f._h for f in fhs])
    assert L.needle_hip_index_add(None, ptrs, 2) == NULL_ARGUMENT
    res = (capi.CSearchResult * 4)()
    assert L.needle_hip_index_results(None, res, 4) == NULL_ARGUMENT
    total, last = C.c_uint64(), C.c_uint64()
    assert L.needle_hip_index_pairs_searched(None, C.byref(total), C.byref(last)) == NULL_ARGUMENT

    index = capi.Index(cmp)
    h = index._h
    assert len(index) == 0 and index.results() == [] and index.pairs_searched() == (0, 0)
    assert L.needle_hip_index_add(h, ptrs, 0) == INVALID_ARGUMENT             # k = 0
    assert L.needle_hip_index_add(h, None, 2) == NULL_ARGUMENT
    holes = (C.c_void_p * 2)(fhs[0]._h, None)
    assert L.needle_hip_index_add(h, holes, 2) == NULL_ARGUMENT              # a NULL FrameHashes among them
    assert L.needle_hip_index_results(h, None, 0) == OK                      # nothing to write for an empty index
    assert L.needle_hip_index_pairs_searched(h, None, None) == OK
    with pytest.raises(capi.NeedleError) as e:
        index.add([])
    assert e.value.name == "InvalidArgument"
    assert len(index) == 0


def test_index_add_fails_cleanly_without_a_gpu(has_gpu):
    """No CPU fallback: the add reports the library's usual error and the index stays empty."""
    if has_gpu:
        pytest.skip("a GPU is present; covered by tests/test_gpu_index.py")
    index = capi.Index(capi.Comparator(["a.mkv", "b.mkv"]))
    with pytest.raises(capi.NeedleError) as e:
        index.add(_frame_hashes(3))
    assert e.value.name == "Unknown" and "no HIP device" in str(e.value)
    assert len(index) == 0 and index.results() == [] and index.pairs_searched() == (0, 0)
    res = (capi.CSearchResult * 1)()
    assert capi.lib().needle_hip_index_results(index._h, res, 1) == OK

