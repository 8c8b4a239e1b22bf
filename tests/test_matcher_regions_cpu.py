"""Regions in the matcher, without a GPU: needle_hip_matcher_new_regions through every layer, its argument checks in the
order "arguments, then device", and the loud failure of creation when there is no device.  What needs an object is in
tests/test_gpu_matcher_regions.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from needle_amd import capi
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NULL = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("NullArgument")


def test_symbol_in_every_layer():
    sym = "needle_hip_matcher_new_regions"
    header = R.strip_comments(open(os.path.join(ROOT, "include", "needle_hip.h")).read())
    lib_rs = open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")).read()
    protos = R.c_prototypes()
    fns, _, _ = R.rust_declarations()
    assert re.search(r"\b%s\s*\(" % sym, header)
    assert hasattr(capi.lib(), sym) and sym in capi.NEEDLE_HIP_H_SYMBOLS
    assert fns[sym] == protos[sym] == (["*const u32", "usize", "*const NeedleHipSeq", "*const u32", "usize", "usize", "usize", "u32",
                                        "*mut *mut NeedleHipMatcher"], "NeedleError")
    assert re.search(r"ffi::%s\(" % sym, lib_rs) and "pub fn with_regions(sources" in lib_rs
    assert callable(capi.Matcher.with_regions)


def _new(lens=(10, 20), min_len=None, regions=1, lanes=2, arena=None, offsets=None, out=True, seqs=True, hashes=True, mins=True, old=False):
    """The raw call over sources of `lens` hashes packed in an arena of `arena` (default: their sum) hashes; `old`: the
    constructor without regions.  Returns (error, handle, message)."""
    h = C.c_void_p()
    table = np.zeros((max(len(lens), 1), 2), dtype=np.uint32)
    table[:len(lens), 1] = lens
    table[:len(lens), 0] = np.cumsum([0] + list(lens))[:len(lens)] if offsets is None else offsets
    arena = sum(lens) if arena is None else arena
    store = np.zeros(max(min(arena, 1 << 20), 1), dtype=np.uint32)              # (a refused call never reads it)
    ml = np.ascontiguousarray(list(min_len if min_len is not None else [3] * len(lens)) or [0], dtype=np.uint32)
    args = [store.ctypes.data if hashes else None, arena, table.ctypes.data if seqs else None, ml.ctypes.data if mins else None, len(lens)]
    tail = [lanes, 10, C.byref(h) if out else None]
    L = capi.lib()
    err = L.needle_hip_matcher_new(*args, *tail) if old else L.needle_hip_matcher_new_regions(*args, regions, *tail)
    return err, h, (L.needle_hip_last_error_message() or b"").decode()


def _refused(words, **kw):
    """InvalidArgument whether or not there is a device: the check comes before it."""
    err, h, said = _new(**kw)
    assert h.value is None and err == INVALID and words in said, (kw, err, said)


def test_creation_checks_its_arguments_before_it_asks_for_a_device():
    for kw in (dict(out=False), dict(seqs=False), dict(mins=False), dict(hashes=False)):
        assert _new(**kw)[0] == NULL, kw
    for regions in (0, 3):
        _refused("regions must be 1 or 2", regions=regions, lens=(10,) * 6, lanes=6)
    _refused("multiples of the regions", regions=2, lens=(10, 20, 30), lanes=2)          # sources
    _refused("multiples of the regions", regions=2, lens=(10, 20), lanes=3)              # lanes
    for lanes in (0, 65536, 65537, 131070):
        _refused("lanes must be 1 to 65535", regions=1, lanes=lanes)
    for lanes in (0, 65536, 131070):                                                     # (65 535 is odd: 65 534 is the most)
        _refused("lanes must be 1 to 65535", regions=2, lanes=lanes)
    _refused("multiples of the regions", regions=2, lanes=65535)
    _refused("1 to 2^32 - 1 sources", lens=())
    _refused("outside the hashes", lens=(10, 20), arena=29)
    _refused("outside the hashes", lens=(10, 20), offsets=[0, 11])
    _refused("outside the hashes", lens=(10, 20, 5, 5), offsets=[0, 10, 2 ** 32 - 1, 30], regions=2)
    for call in (lambda: capi.Matcher.with_regions([np.zeros(4, np.uint32)] * 2, [1, 1], 3, 2, 10),
                 lambda: capi.Matcher.with_regions([np.zeros(4, np.uint32)] * 3, [1, 1, 1], 2, 2, 10),
                 lambda: capi.Matcher.with_regions([np.zeros(4, np.uint32)] * 2, [1, 1], 2, 1, 10),
                 lambda: capi.Matcher.with_regions([np.zeros(4, np.uint32)] * 2, [1, 1], 2, 65536, 10)):
        with pytest.raises(capi.NeedleError) as e:
            call()
        assert e.value.code == INVALID
    with pytest.raises(ValueError):
        capi.Matcher.with_regions([np.zeros(4, np.uint32)] * 2, [1], 2, 2, 10)


def test_one_region_refuses_what_the_old_constructor_refuses():
    """The same error and the same words from both, for every refusal the two share; a min_len of 0 is the one difference,
    and the old constructor keeps refusing it."""
    shared = (dict(lanes=0), dict(lanes=65536), dict(lens=()), dict(lens=(10, 20), arena=29), dict(lens=(10, 20), offsets=[0, 11]),
              dict(out=False), dict(seqs=False), dict(mins=False), dict(hashes=False))
    for kw in shared:
        old, new = _new(old=True, **kw), _new(regions=1, **kw)
        assert old[0] == new[0] and old[0] in (INVALID, NULL), kw
        assert old[1].value is None and new[1].value is None
        if old[0] == INVALID:
            assert old[2] == new[2], kw
    err, h, said = _new(old=True, min_len=(3, 0))
    assert err == INVALID and h.value is None and "min_len must be >= 1" in said


ACCEPTED = [dict(regions=1, lens=(10, 20), lanes=1),
            dict(regions=1, lens=(10, 20), min_len=(3, 0), lanes=3),                     # a source that can hold no run
            dict(regions=2, lens=(1030, 37, 300, 0, 2, 257), lanes=4),
            dict(regions=2, lens=(0, 1), min_len=(0, 0), lanes=2),                       # no source has a cell
            dict(regions=2, lens=(10, 20), lanes=65534)]


def test_creation_without_a_device_fails_loudly():
    """What passes the checks reaches the device: with one the object exists, without one the failure says so."""
    for kw in ACCEPTED:
        if kw["lanes"] > 1000 and capi.device_count() > 0:
            continue                                                                     # (65 534 lanes of state: the checks are the point)
        err, h, said = _new(**kw)
        if capi.device_count() > 0:
            assert err == 0 and h.value, kw
            capi.lib().needle_hip_matcher_free(h)
        else:
            assert err not in (0, INVALID, NULL) and h.value is None, kw
            assert "no HIP device" in said, kw
    if capi.device_count() > 0:
        return
    with pytest.raises(capi.NeedleError) as e:
        capi.Matcher.with_regions([np.arange(10, dtype=np.uint32)] * 2, [2, 2], 2, 2, 10)
    assert "no HIP device" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:                                           # argument errors come first, device or not
        capi.Matcher.with_regions([np.arange(10, dtype=np.uint32)] * 2, [2, 2], 2, 3, 10)
    assert "multiples of the regions" in str(e.value)
