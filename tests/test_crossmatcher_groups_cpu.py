"""Groups of videos in the cross-matcher and the streamed route into a grouped index, without a GPU: the live-pair table
builder (needle_amd/csrc/cross_pairs.h) against brute force in a stand-alone program, plain and under AddressSanitizer and
UndefinedBehaviorSanitizer; the new entry points through every layer; their argument checks, which come before a device is
asked for; the state-size arithmetic; and the NumPy model of the grouped ids (tests/group_ids.py) against
needle_hip_group_pairs for the label patterns tests/test_gpu_crossmatcher_groups.py uses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from needle_amd import capi
from tests import group_ids as G
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["needle_hip_crossmatcher_new_grouped", "needle_hip_crossmatcher_state_bytes_grouped", "needle_hip_crossmatcher_groups",
           "needle_hip_index_crossmatcher_new_grouped", "needle_hip_index_add_matched_grouped"]
INVALID, NULL = capi.ERROR_NAMES.index("InvalidArgument"), capi.ERROR_NAMES.index("NullArgument")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_the_live_pair_table_against_brute_force(tmp_path, flags):
    """tests/cpp/cross_pairs_check.cpp: every assignment of <= 3 labels to V <= 7 videos, every K <= V - 1, regions 1 and 2."""
    exe = str(tmp_path / "cross_pairs_check")
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "needle_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "cross_pairs_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("cross pairs ok"), out.stdout[-2000:] + out.stderr[-4000:]
    cases = sum(3 ** v * v * 2 for v in range(1, 8))                             # V videos: 3^V labellings x K = 0 .. V - 1 x 2
    assert out.stdout.splitlines()[0] == f"{cases} cases"
    # ... and the plan of a shape without labels against the object as it was before one plan served both: accepted layouts
    # field by field (K <= 4, N <= 5), and 8 K x 5 N x 4 regions x 6 max_items x 2 rows boundary shapes refusal by refusal
    layouts, boundaries = out.stdout.splitlines()[1:3]
    assert re.fullmatch(r"[1-9]\d* unlabelled layouts", layouts) and boundaries == f"{8 * 5 * 4 * 6 * 2} boundary shapes"


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
    assert protos["needle_hip_crossmatcher_new_grouped"] == (
        ["*const u32", "usize", "*const NeedleHipSeq", "usize", "*const u32", "usize", "*const u32", "usize", "*const usize", "*const u32",
         "u32", "*mut *mut NeedleHipCrossMatcher"], "NeedleError")
    assert protos["needle_hip_index_crossmatcher_new_grouped"] == (
        ["*mut NeedleHipIndex", "usize", "*const u32", "*const usize", "*const u32", "*mut *mut NeedleHipCrossMatcher"], "NeedleError")
    for name in ("with_groups", "state_bytes_grouped"):
        assert callable(getattr(capi.CrossMatcher, name)), name
    assert isinstance(capi.CrossMatcher.groups, property)
    for name in ("pub fn with_groups(", "pub fn groups(", "pub fn state_bytes_grouped(", "pub fn crossmatcher_grouped(",
                 "pub fn add_matched_grouped("):
        assert name in lib_rs, name


def _new(lens=(10, 20), res_groups=(1, 2), groups=(1, 2, 1), max_items=(100,), min_len=(8,), regions=None, arena=None, out=True,
         seqs=True, hashes=True, labels=True, res_labels=True):
    """The raw call.  Returns (error, handle, message)."""
    h = C.c_void_p()
    regions = len(max_items) if regions is None else regions
    table = np.zeros((max(len(lens), 1), 2), dtype=np.uint32)
    table[:len(lens), 1] = lens
    table[:len(lens), 0] = np.cumsum([0] + list(lens))[:len(lens)]
    arena = sum(lens) if arena is None else arena
    store = np.zeros(max(min(arena, 1 << 20), 1), dtype=np.uint32)               # (a refused call never reads it)
    mi = None if max_items is None else (C.c_size_t * max(len(max_items), 1))(*max_items)
    ml = None if min_len is None else (C.c_uint32 * max(len(min_len), 1))(*min_len)
    g = np.ascontiguousarray(list(groups) or [0], dtype=np.uint32)             # (no videos: still an array, the count is what is refused)
    rg = np.ascontiguousarray(res_groups, dtype=np.uint32)
    err = capi.lib().needle_hip_crossmatcher_new_grouped(
        store.ctypes.data if hashes and arena else None, arena, table.ctypes.data if seqs else None, len(res_groups),
        rg.ctypes.data if res_labels and rg.size else None, len(groups), g.ctypes.data if labels else None, regions, mi, ml, 10,
        C.byref(h) if out else None)
    return err, h, (capi.lib().needle_hip_last_error_message() or b"").decode()


def _refused(words, **kw):
    """InvalidArgument whether or not there is a device: the check comes before it."""
    err, h, message = _new(**kw)
    assert h.value is None and err == INVALID and words in message, (err, message)
    return True


def test_creation_checks_its_arguments_before_it_asks_for_a_device():
    assert _new(out=False)[0] == NULL
    assert _new(max_items=None, regions=1)[0] == NULL
    assert _new(min_len=None)[0] == NULL
    assert _new(seqs=False)[0] == NULL
    assert _new(hashes=False)[0] == NULL
    assert _new(labels=False)[0] == NULL                                         # labels missing
    assert _new(res_labels=False)[0] == NULL
    for regions in (0, 3):
        assert _refused("regions must be 1 or 2", lens=(10,) * 6, res_groups=(1, 2), regions=regions, max_items=(100, 50, 25), min_len=(8, 5, 3))
    assert _refused("arriving videos must be 1 to 256", groups=())
    assert _refused("arriving videos must be 1 to 256", groups=(1,) * 257)
    assert _refused("max_items must be 2", max_items=(1,))
    assert _refused("min_len must be >= 1", min_len=(0,))
    assert _refused("outside the hash arena", arena=29)
    # the bound is on the LIVE problems: 65 536 residents of the arriving video's label are refused ...
    many = 65536
    assert _refused("more than 65 535 live problems", lens=(2,) * many, res_groups=(5,) * many, groups=(5,))
    assert _refused("more than 65 535 live problems", lens=(2,) * many, res_groups=(5,) * (many // 2), groups=(5,), max_items=(9, 9), min_len=(2, 2))
    assert _refused("more than 65 535 live problems", lens=(2,) * 255, res_groups=(5,) * 255, groups=(5,) * 256)
    sb = capi.CrossMatcher.state_bytes_grouped
    assert sb((5,), (9,), (2,) * many, (5,) * many) == 0
    # ... and the same residents under another label are no live problem at all
    assert sb((6,), (9,), (2,) * many, (5,) * many) == 1 * 9 * 4
    for call in (lambda: capi.CrossMatcher.with_groups([], [10], [1], 10),
                 lambda: capi.CrossMatcher.with_groups([1, 1], [10], [0], 10),
                 lambda: capi.CrossMatcher.with_groups([1] * 257, [10], [1], 10)):
        with pytest.raises(capi.NeedleError) as e:
            call()
        assert e.value.code in (INVALID, NULL)
    with pytest.raises(ValueError):
        capi.CrossMatcher.with_groups([1, 1], [10, 10], [1, 1], 10, resident=[np.zeros(4, np.uint32)] * 3, resident_groups=[1, 1])


def test_creation_without_a_device_fails_loudly():
    """What passes the checks reaches the device: with one the object exists, without one the failure says so."""
    for kw in (dict(), dict(lens=(), res_groups=(), groups=(1, 2)), dict(lens=(), res_groups=(), groups=(3,)),
               dict(lens=(2,) * 65535, res_groups=(5,) * 65535, groups=(5,))):   # no live pair at all; exactly 65 535
        err, h, message = _new(**kw)
        if capi.device_count() > 0:
            assert err == 0 and h.value, kw
            n = len(kw.get("res_groups", (1, 2))) + len(kw.get("groups", (1, 2, 1)))
            got = (C.c_uint32 * n)()
            assert capi.lib().needle_hip_crossmatcher_groups(h, got, n) == 0
            assert list(got) == list(kw.get("res_groups", (1, 2))) + list(kw.get("groups", (1, 2, 1)))
            assert capi.lib().needle_hip_crossmatcher_groups(h, got, n - 1) == INVALID
            capi.lib().needle_hip_crossmatcher_free(h)
        else:
            assert err not in (0, INVALID, NULL) and h.value is None, kw
            assert "no HIP device" in message, kw
    assert capi.lib().needle_hip_crossmatcher_groups(None, (C.c_uint32 * 1)(), 1) == NULL


def _formula(groups, max_items, lens, res_groups):
    """Frontiers and hashes for live pairs only."""
    regions, k = len(max_items), len(res_groups)
    labels = list(res_groups) + list(groups)
    live = G.live_pairs(labels, k)
    live_res = sorted({a for a, b in live if a < k})
    w = 2 if all(x < 65536 for x in max_items) and all(lens[a * regions + r] < 65536 for a in live_res for r in range(regions)) else 4
    arriving = sum(1 for a, b in live if a >= k)
    total = 0
    for r in range(regions):
        total += arriving * 4 * max_items[r] * w + len(groups) * max_items[r] * 4
        total += sum(2 * lens[a * regions + r] * w for a, b in live if a < k) + sum(lens[a * regions + r] * 4 for a in live_res)
    return total


@pytest.mark.parametrize("groups,max_items,lens,res_groups", [
    ((1, 2, 1, 2, 3), (100,), (), ()),
    ((1, 2, 1), (100,), (10, 20, 30), (1, 2, 9)),
    ((0, 0xFFFFFFFF, 0), (100, 60), (10, 20, 30, 40), (0xFFFFFFFF, 4)),
    ((7, 7), (48,), (65536, 10), (7, 8)), ((7, 7), (48,), (10, 65536), (7, 8)),   # only a LIVE resident widens the entries
    ((3,), (9,), (), ())])
def test_state_bytes_grouped_is_the_formula(groups, max_items, lens, res_groups):
    got = capi.CrossMatcher.state_bytes_grouped(groups, max_items, lens, res_groups)
    assert got == _formula(groups, max_items, lens, res_groups) > 0


def test_state_bytes_grouped_against_the_ungrouped_formulas():
    sb, sbg = capi.CrossMatcher.state_bytes, capi.CrossMatcher.state_bytes_grouped
    assert sbg((4,) * 5, (100, 60)) == sb(5, (100, 60))                          # one label, no residents: the regions call
    assert sbg((4,) * 3, (48,), (10, 0, 7), (4,) * 3) == sb(3, (48,), (10, 0, 7))   # one label: the resident call
    assert sbg((1, 2, 3), (48,)) == 3 * 48 * 4                                   # nobody has a partner: the histories alone
    # a resident nobody arrives for costs nothing, with or without it in the list
    assert sbg((1, 1), (48,), (10, 500, 20), (1, 9, 1)) == sbg((1, 1), (48,), (10, 20), (1, 1))
    # 16 shows of 16 against one show of 256, lanes of 5 441 items: 1 920 live pairs against 32 640
    assert sbg([v // 16 for v in range(256)], (5441,)) == 1920 * 4 * 5441 * 2 + 256 * 5441 * 4 < sb(256, 5441) == 32640 * 4 * 5441 * 2 + 256 * 5441 * 4
    assert capi.lib().needle_hip_crossmatcher_state_bytes_grouped(None, 0, None, 2, None, 1, (C.c_size_t * 1)(10)) == 0
    assert capi.lib().needle_hip_crossmatcher_state_bytes_grouped(None, 2, None, 2, (C.c_uint32 * 2)(1, 1), 1, (C.c_size_t * 1)(10)) == 0


def test_the_index_entry_points_check_their_arguments():
    cmp = capi.Comparator(["a.mkv", "b.mkv"], hash_match_threshold=10, min_opening_duration=10)
    plain, grouped = capi.Index(cmp), capi.Index(cmp, grouped=True)
    L = capi.lib()
    h = C.c_void_p()
    one, labels = (C.c_size_t * 1)(100), (C.c_uint32 * 2)(1, 1)
    ml = (C.c_uint32 * 1)(8)
    new = L.needle_hip_index_crossmatcher_new_grouped
    assert new(None, 2, labels, one, ml, C.byref(h)) == NULL
    assert new(grouped._h, 2, None, one, ml, C.byref(h)) == NULL
    assert new(grouped._h, 2, labels, None, ml, C.byref(h)) == NULL
    assert new(grouped._h, 2, labels, one, None, C.byref(h)) == NULL
    assert new(grouped._h, 2, labels, one, ml, None) == NULL
    assert new(plain._h, 2, labels, one, ml, C.byref(h)) == INVALID and h.value is None
    assert "not a grouped index" in L.needle_hip_last_error_message().decode()
    assert new(grouped._h, 0, labels, one, ml, C.byref(h)) == INVALID
    assert new(grouped._h, 257, (C.c_uint32 * 257)(), one, ml, C.byref(h)) == INVALID
    assert "arriving videos must be 1 to 256" in L.needle_hip_last_error_message().decode()
    assert new(grouped._h, 2, labels, one, (C.c_uint32 * 1)(0), C.byref(h)) == INVALID
    assert "min_len" in L.needle_hip_last_error_message().decode()
    with pytest.raises(capi.NeedleError, match="not a grouped index"):
        plain.crossmatcher(2, [100], [8], groups=[1, 1])
    with pytest.raises(capi.NeedleError, match="no streamed routes"):            # without groups= the old entry point, refused as before
        grouped.crossmatcher(2, [100], [8])
    with pytest.raises(ValueError):
        grouped.crossmatcher(2, [100], [8], groups=[1])
    add = L.needle_hip_index_add_matched_grouped
    fake = C.c_void_p(1)                                                         # (never looked into: the checks below come first)
    assert add(None, fake, None, 1) == NULL and add(grouped._h, None, None, 1) == NULL
    assert add(grouped._h, fake, None, 0) == INVALID and "no videos" in L.needle_hip_last_error_message().decode()
    assert add(grouped._h, fake, None, 1) == NULL
    assert len(plain) == 0 and len(grouped) == 0 and grouped.groups() == []


@pytest.mark.parametrize("labels", [
    [1, 2] * 6 + [3],                                                            # the two interleaved seasons and one lane alone
    [0, 0xFFFFFFFF, 0, 5, 0xFFFFFFFF],                                           # two regions: members not adjacent
    [1, 2, 9, 1, 2, 1, 2, 7, 2],                                                 # five residents over three labels, four arriving
    [1, 2, 1, 2, 1, 2, 7, 2],                                                    # ... without the resident nobody arrives for
    [4, 4, 6, 6],
    list(range(300)) + [t // 4 for t in range(256)]])                            # the bounds case
def test_the_id_model_is_needle_hip_group_pairs(labels):
    got = [tuple(int(x) for x in p) for p in capi.group_pairs(labels)]
    assert got == G.pairs(labels)
    for k, (a, b) in enumerate(got):
        assert G.pair_id(labels, a, b) == k
