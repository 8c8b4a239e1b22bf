"""CPU tests of a library over groups of videos (needle_hip_library_set_groups / _groups, include/needle_hip.h): the
symbols, the grouped pair count for labellings that take every edge of the numbering, the refusals that are decided before
any device is asked for, and the labels' round trip.  (The refusal of a call AFTER set_pcm / set_pcm_device / stream_pcm
needs PCM on a device: tests/test_gpu_library_groups.py.)"""
import ctypes as C
import os
import re

import pytest

from needle_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL_ARGUMENT, INVALID_ARGUMENT = 0, capi.ERROR_NAMES.index("NullArgument"), capi.ERROR_NAMES.index("InvalidArgument")
SYMBOLS = ["needle_hip_library_set_groups", "needle_hip_library_groups"]

LABELLINGS = {
    "adjacent members": [1, 1, 1, 2, 2, 3, 3, 3, 3],
    "scattered members": [5, 9, 5, 7, 9, 5, 3, 9],
    "a group of one between two others": [4, 4, 8, 6, 6, 6],  # the shared-base bisection edge: base[8] == base[6]
    "a group of one first and last": [0, 2, 2, 2, 0xFFFFFFFF],
    "all videos alone": [10, 11, 12, 13, 14],
    "one label for all": [7] * 6,
    "one video": [3],
}


def _expected_pairs(labels):
    sizes = {}
    for g in labels:
        sizes[g] = sizes.get(g, 0) + 1
    return sum(k * (k - 1) // 2 for k in sizes.values())


def test_symbols_are_declared_exported_bound_and_named_in_rust():
    with open(os.path.join(ROOT, "include", "needle_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "rust", "needle-hip", "src", "ffi.rs")) as f:
        ffi = f.read()
    with open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")) as f:
        wrapper = f.read()
    for name in SYMBOLS:
        assert name + "(" in header
        assert name in capi.NEEDLE_HIP_H_SYMBOLS
        assert hasattr(capi.lib(), name)
        assert getattr(capi.lib(), name).argtypes is not None, "bound with its argument types"
        assert re.search(r"pub fn %s\(" % name, ffi) and "ffi::%s(" % name in wrapper
    assert "the library job and the" not in header, "the header no longer says that the library job takes no groups"


def test_the_rust_declarations_match_the_header():
    from tests import rust_ffi_check as R
    protos, (fns, _, _) = R.c_prototypes(), R.rust_declarations()
    for name in SYMBOLS:
        assert fns[name] == protos[name], (name, fns[name], protos[name])


@pytest.mark.parametrize("name", list(LABELLINGS))
def test_num_pairs_is_the_grouped_pair_count(name):
    labels = LABELLINGS[name]
    library = capi.Library(len(labels))
    assert library.num_pairs() == len(labels) * (len(labels) - 1) // 2, "a plain library: all pairs"
    assert library.set_groups(labels) is library
    want = len(capi.group_pairs(labels))
    assert want == _expected_pairs(labels)
    assert library.num_pairs() == want
    assert library.groups() == labels, "the labels round-trip"
    # labels can be replaced while there is no PCM
    library.set_groups(list(range(len(labels))))
    assert library.num_pairs() == 0 and library.groups() == list(range(len(labels)))


def test_one_label_is_the_plain_pair_count():
    library = capi.Library(9).set_groups([42] * 9)
    assert library.num_pairs() == 36 == capi.Library(9).num_pairs()


def test_refusals_leave_the_library_unchanged():
    L = capi.lib()
    library = capi.Library(4)
    labels = (C.c_uint32 * 5)(1, 1, 2, 2, 2)
    out = (C.c_uint32 * 5)()
    # NULL arguments
    assert L.needle_hip_library_set_groups(None, labels, 4) == NULL_ARGUMENT
    assert L.needle_hip_library_set_groups(library._h, None, 4) == NULL_ARGUMENT
    assert L.needle_hip_library_groups(None, out, 4) == NULL_ARGUMENT
    assert L.needle_hip_library_groups(library._h, None, 4) == NULL_ARGUMENT
    # a plain library has no labels, as needle_hip_index_groups of a plain index
    assert L.needle_hip_library_groups(library._h, out, 4) == INVALID_ARGUMENT
    with pytest.raises(capi.NeedleError):
        library.groups()
    # a number of videos other than the library's
    for k in (0, 3, 5):
        assert L.needle_hip_library_set_groups(library._h, labels, k) == INVALID_ARGUMENT
        assert library.num_pairs() == 6 and L.needle_hip_library_groups(library._h, out, 4) == INVALID_ARGUMENT, "still plain"
    with pytest.raises(capi.NeedleError):
        library.set_groups([1, 2, 3])
    assert L.needle_hip_library_set_groups(library._h, labels, 4) == OK
    assert library.num_pairs() == 2 and library.groups() == [1, 1, 2, 2]
    # ... and a refused call changes nothing on a grouped library either
    assert L.needle_hip_library_set_groups(library._h, labels, 5) == INVALID_ARGUMENT
    assert L.needle_hip_library_set_groups(library._h, None, 4) == NULL_ARGUMENT
    assert library.num_pairs() == 2 and library.groups() == [1, 1, 2, 2]
    # too few slots for the labels
    assert L.needle_hip_library_groups(library._h, out, 3) == INVALID_ARGUMENT
    assert L.needle_hip_library_groups(library._h, out, 5) == OK and list(out[:4]) == [1, 1, 2, 2]
