"""CPU: chromaprint's fingerprint codec.  The model (tests/fp_codec.py) against the format's ten vectors and itself; the new
entry points in every layer; the pure-host calls (bound, base64, tiles, simhash) against the model and Python's base64; the
compute calls without a device; and tests/cpp/fp_codec_check.cpp -- the shared index arithmetic of
needle_amd/csrc/fp_codec.h driven through a sequential emulation of the device passes over exactly-sized buffers --
once as it is and once under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program)."""
import base64
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from needle_amd import capi
from oracle import oracle as O
from tests import fp_codec as M
from tests import rust_ffi_check as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_SYMBOLS = ["needle_hip_fingerprint_compressed_bound", "needle_hip_fingerprint_compress_host",
               "needle_hip_fingerprint_decompress_host", "needle_hip_feeder_compressed",
               "needle_hip_fingerprint_base64_encode", "needle_hip_fingerprint_base64_decode",
               "needle_hip_fingerprint_codec_tiles", "needle_hip_fingerprint_simhash"]
CHROMAPRINT_SYMBOLS = ["chromaprint_get_fingerprint", "chromaprint_get_fingerprint_hash", "chromaprint_encode_fingerprint",
                       "chromaprint_decode_fingerprint", "chromaprint_hash_fingerprint"]


def test_model_reproduces_the_ten_vectors():
    for items, algorithm, want in M.VECTORS:
        assert list(M.compress(items, algorithm)) == want, items
        assert M.decompress(bytes(want)) == (items, algorithm, M.OK)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "chromaprint_silence.json")))
    assert M.SILENCE_TEXT in json.dumps(golden)
    assert M.b64encode(M.compress(M.SILENCE_ITEMS, M.SILENCE_ALGORITHM)) == M.SILENCE_TEXT
    assert M.decompress(M.b64decode(M.SILENCE_TEXT)) == (M.SILENCE_ITEMS, M.SILENCE_ALGORITHM, M.OK)
    assert len(M.VECTORS) + 1 == 10


def test_model_round_trips_and_refuses():
    rng = np.random.default_rng(5)
    for n in [0, 1, 2, 33, 500]:
        deltas = [int(sum(1 << int(b) for b in set(rng.integers(0, 32, rng.integers(0, 9))))) for _ in range(n)]
        items = np.bitwise_xor.accumulate(np.array(deltas, dtype=np.uint32)).tolist() if n else []
        blob = M.compress(items, 3)
        assert M.decompress(blob) == (items, 3, M.OK)
        assert M.decompress(blob + b"\xff\x01") == (items, 3, M.OK)              # trailing bytes are ignored
        normal, exceptional = M.symbols(items)
        assert len(blob) == 4 + (3 * len(normal) + 7) // 8 + (5 * len(exceptional) + 7) // 8
    blob = M.compress([0x80000001, 1 << 8, 7], 1)
    statuses = [M.decompress(blob[:k])[2] for k in range(len(blob) + 1)]
    assert statuses[:4] == [M.SHORT_HEADER] * 4 and statuses[-1] == M.OK
    assert set(statuses[4:-1]) == {M.NORMAL_ENDS, M.EXCEPTIONAL_ENDS} and statuses[4:-1] == sorted(statuses[4:-1])
    assert M.decompress(bytes([0, 0xFF, 0xFF, 0xFF]))[2] == M.NORMAL_ENDS
    assert M.decompress(bytes([0, 0, 0, 1, 15, 0, 25])) == ([], 0, M.BIT_POSITION)   # gaps 32 + 1


def test_new_symbols_in_every_layer():
    """Declared in both headers, exported by both libraries, listed in capi.NEEDLE_HIP_H_SYMBOLS, declared in ffi.rs with
    the header's types, wrapped in lib.rs."""
    L = capi.lib()
    hip_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "needle_hip.h")).read(), flags=re.S)
    chroma_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "needle_chromaprint.h")).read(), flags=re.S)
    CL = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libneedle_chromaprint.so"))
    protos = R.c_prototypes()
    fns, _, _ = R.rust_declarations()
    lib_rs = open(os.path.join(ROOT, "rust", "needle-hip", "src", "lib.rs")).read()
    for sym in HIP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, hip_h), sym
        assert hasattr(L, sym), sym
        assert sym in capi.NEEDLE_HIP_H_SYMBOLS, sym
        assert sym in fns and fns[sym] == protos[sym], (sym, fns.get(sym), protos[sym])
        assert "ffi::" + sym in lib_rs, sym
    for sym in CHROMAPRINT_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, chroma_h), sym
        assert hasattr(CL, sym), sym


def test_compressed_bound_against_the_model():
    assert [capi.fingerprint_compressed_bound(n) for n in (0, 1, 2, 3)] == [4, 4 + 13 + 3, 4 + 25 + 5, 4 + 38 + 8]
    for n in [1, 2, 7, 8, 1000]:
        bound = capi.fingerprint_compressed_bound(n)
        assert bound == 4 + (99 * n + 7) // 8 + (20 * n + 7) // 8
        dense = [0xFFFFFFFF if i % 2 == 0 else 0 for i in range(n)]                          # x all ones: 33 symbols an item
        assert len(M.compress(dense)) == 4 + (99 * n + 7) // 8 <= bound
        x = (1 << 6) | (1 << 13) | (1 << 20) | (1 << 27)                                     # four gaps of 7: 4 exceptional
        four = [x if i % 2 == 0 else 0 for i in range(n)]
        assert len(M.compress(four)) == 4 + (15 * n + 7) // 8 + (20 * n + 7) // 8 <= bound
    t, d = capi.fingerprint_codec_tiles()
    assert t >= 64 and d >= 64


def test_base64_against_pythons():
    rng = np.random.default_rng(7)
    for n in range(10):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        text = capi.fingerprint_base64_encode(data)
        assert text == base64.urlsafe_b64encode(data).decode().rstrip("=") == M.b64encode(data)
        assert capi.fingerprint_base64_decode(text) == data
    assert capi.fingerprint_base64_encode(b"\xfb\xff\xfe") == "-__-"
    assert capi.fingerprint_base64_decode("-__-") == b"\xfb\xff\xfe"
    for bad in ["A", "AAAAA", "AA=A", "AA==", "AA+A", "AA/A", "AA A", "AAA\n"]:
        assert M.b64decode(bad) is None
        with pytest.raises(capi.NeedleError, match="InvalidArgument"):
            capi.fingerprint_base64_decode(bad)
    # NULL arguments
    L = capi.lib()
    assert L.needle_hip_fingerprint_base64_encode(None, 0, None, None) == capi.ERROR_NAMES.index("NullArgument")
    assert L.needle_hip_fingerprint_codec_tiles(None, None) == capi.ERROR_NAMES.index("NullArgument")


def test_simhash_is_the_oracles():
    rng = np.random.default_rng(11)
    for n in [0, 1, 2, 63, 64, 65, 1000]:
        fp = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        assert capi.fingerprint_simhash(fp) == O.simhash32(fp.tolist())
    assert capi.fingerprint_simhash([]) == 0


def test_compute_calls_need_a_device_and_check_their_arguments(has_gpu):
    L = capi.lib()
    NULL, INVALID = capi.ERROR_NAMES.index("NullArgument"), capi.ERROR_NAMES.index("InvalidArgument")
    off = (C.c_uint64 * 2)(0, 0)
    out_off = (C.c_uint64 * 2)()
    ptr = C.c_void_p()
    assert L.needle_hip_fingerprint_compress_host(None, None, 0, 1, C.byref(ptr), out_off) == NULL
    assert L.needle_hip_fingerprint_compress_host(None, off, 1, 1, None, out_off) == NULL
    assert L.needle_hip_fingerprint_decompress_host(None, off, 1, C.byref(ptr), out_off, None, None) == NULL
    assert L.needle_hip_feeder_compressed(None, 0, 1, C.byref(ptr), C.byref(C.c_size_t())) == NULL
    # refused before a device is asked for: offsets that decrease, a fingerprint the header cannot count
    bad = (C.c_uint64 * 3)(0, 5, 3)
    items = np.zeros(8, np.uint32)
    assert L.needle_hip_fingerprint_compress_host(items.ctypes.data, bad, 2, 1, C.byref(ptr), (C.c_uint64 * 3)()) == INVALID
    alg, st = np.zeros(2, np.int32), np.zeros(2, np.int32)
    assert L.needle_hip_fingerprint_decompress_host(items.ctypes.data, bad, 2, C.byref(ptr), (C.c_uint64 * 3)(), alg.ctypes.data,
                                                    st.ctypes.data) == INVALID
    huge = (C.c_uint64 * 2)(0, 1 << 24)
    assert L.needle_hip_fingerprint_compress_host(items.ctypes.data, huge, 1, 1, C.byref(ptr), out_off) == INVALID
    if not has_gpu:
        with pytest.raises(capi.NeedleError, match="no HIP device"):
            capi.compress_fingerprints([[1, 2, 3]])
        with pytest.raises(capi.NeedleError, match="no HIP device"):
            capi.decompress_fingerprints([bytes([0, 0, 0, 1, 1])])
        CL = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libneedle_chromaprint.so"))
        CL.chromaprint_encode_fingerprint.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int]
        size = C.c_int()
        assert CL.chromaprint_encode_fingerprint(items.ctypes.data, 3, 1, C.byref(ptr), C.byref(size), 1) == 0
        CL.chromaprint_hash_fingerprint.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
        h = C.c_uint32(7)
        assert CL.chromaprint_hash_fingerprint(items.ctypes.data, 8, C.byref(h)) == 1 and h.value == 0


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_index_arithmetic_through_the_emulated_passes(tmp_path, flags):
    exe = str(tmp_path / "fp_codec_check")
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "needle_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "fp_codec_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("fp codec ok"), out.stdout[-4000:] + out.stderr[-4000:]
