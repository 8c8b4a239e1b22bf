"""A streamed season into the index, without a GPU: needle_hip_index_crossmatcher_new, needle_hip_index_add_matched and
needle_hip_index_pairs_scanned through every layer, their NULL checks, the loud failure of creation when there is no
device, and the pair-id arithmetic the ingest kernel runs per run (needle_amd/csrc/pair_ids.h), compiled for the host.
What needs a device is in tests/test_gpu_index_matched.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from needle_amd import capi
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["needle_hip_index_crossmatcher_new", "needle_hip_index_add_matched", "needle_hip_index_pairs_scanned"]
INVALID, NULL = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("NullArgument")


def _index(endings=False):
    return capi.Index(capi.Comparator(["a.mkv", "b.mkv"], include_endings=endings))


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
    assert protos["needle_hip_index_crossmatcher_new"] == (
        ["*mut NeedleHipIndex", "usize", "*const usize", "*const u32", "*mut *mut NeedleHipCrossMatcher"], "NeedleError")
    assert protos["needle_hip_index_add_matched"] == (
        ["*mut NeedleHipIndex", "*mut NeedleHipCrossMatcher", "*const *const FrameHashes", "usize"], "NeedleError")
    assert protos["needle_hip_index_pairs_scanned"] == (["*const NeedleHipIndex", "*mut u64", "*mut u64"], "NeedleError")
    for name in ("crossmatcher", "add_matched", "pairs_scanned"):
        assert callable(getattr(capi.Index, name)), name
    for name in ("pub fn crossmatcher(", "pub fn add_matched(", "pub fn pairs_scanned("):
        assert name in lib_rs, name


def test_rust_declarations_still_match_the_headers():
    protos = R.c_prototypes()
    fns, _, variants = R.rust_declarations()
    for name, (params, ret) in fns.items():
        assert name in protos, name
        assert (params, ret) == protos[name], (name, params, ret, protos[name])
    assert variants == R.header_error_variants()


def test_null_arguments():
    L = capi.lib()
    index = _index()
    one = (C.c_size_t * 1)(100)
    low = (C.c_uint32 * 1)(8)
    h = C.c_void_p()
    assert L.needle_hip_index_crossmatcher_new(None, 2, one, low, C.byref(h)) == NULL
    assert L.needle_hip_index_crossmatcher_new(index._h, 2, None, low, C.byref(h)) == NULL
    assert L.needle_hip_index_crossmatcher_new(index._h, 2, one, None, C.byref(h)) == NULL
    assert L.needle_hip_index_crossmatcher_new(index._h, 2, one, low, None) == NULL
    assert h.value is None
    fh = capi.FrameHashes.new([(1, 0), (2, 1)], [], 0)
    ptrs = (C.c_void_p * 1)(fh._h)
    assert L.needle_hip_index_add_matched(None, None, ptrs, 1) == NULL
    assert L.needle_hip_index_add_matched(index._h, None, ptrs, 1) == NULL           # no matcher
    total, last = C.c_uint64(7), C.c_uint64(7)
    assert L.needle_hip_index_pairs_scanned(None, C.byref(total), C.byref(last)) == NULL
    assert L.needle_hip_index_pairs_scanned(index._h, None, None) == 0               # either pointer may be NULL
    assert L.needle_hip_index_pairs_scanned(index._h, C.byref(total), C.byref(last)) == 0
    assert (total.value, last.value) == (0, 0) == index.pairs_scanned()
    assert len(index) == 0 and index.pairs_searched() == (0, 0)


def test_creation_checks_its_arguments_then_asks_for_a_device():
    """As the other device objects: what the argument checks refuse is InvalidArgument with or without a device; what passes
    them reaches the device, and without one the failure says so."""
    index = _index()
    for videos, max_items, min_len in ((1, [100], [8]), (0, [100], [8]), (257, [100], [8]),   # an empty index is K = 0: 2 .. 256
                                       (3, [1], [8]), (3, [100], [0])):
        with pytest.raises(capi.NeedleError) as e:
            index.crossmatcher(videos, max_items, min_len)
        assert e.value.code == INVALID, (videos, max_items, min_len)
    with pytest.raises(ValueError):
        index.crossmatcher(3, [100, 50], [8])
    if capi.device_count() > 0:
        m = index.crossmatcher(3, [100], [8])
        assert m.shape() == (3, 1) and m.resident == 0 and m.lanes == 3
        assert m.threshold == capi.DEFAULT_HASH_MATCH_THRESHOLD and m.max_items == (100,) and m.min_len == (8,)
        two = _index(endings=True).crossmatcher(2, [100, 50], [8, 5])
        assert two.shape() == (2, 2) and two.lanes == 4
        return
    with pytest.raises(capi.NeedleError) as e:
        index.crossmatcher(3, [100], [8])
    assert e.value.code not in (INVALID, NULL) and "no HIP device" in str(e.value)
    with pytest.raises(capi.NeedleError) as e:                                       # the regions are the index's
        _index(endings=True).crossmatcher(2, [100, 50], [8, 5])
    assert "no HIP device" in str(e.value)


def test_pair_ids_against_the_enumerations(tmp_path):
    """tests/cpp/pair_ids_check.cpp: decode and re-tag of the shared header against brute force, every V <= 48, K <= V,
    R in {1, 2}, and the largest V whose problem index fits 32 bits."""
    exe = str(tmp_path / "pair_ids_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "needle_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "pair_ids_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("pair ids ok"), out.stdout + out.stderr
