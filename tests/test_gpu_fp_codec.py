"""GPU: chromaprint's fingerprint codec on the device (needle_amd/csrc/fp_codec.hip) against the model of tests/fp_codec.py,
byte for byte: upstream's silence string end to end through the libchromaprint layer, the format's ten vectors, the
edges of both tiles, the refusals beside good blobs, a feeder's lanes, and the hash."""
import ctypes as C
import os

import numpy as np
import pytest

from needle_amd import capi
from oracle import oracle as O
from tests import fp_codec as M

pytestmark = pytest.mark.gpu


def _chromaprint():
    L = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libneedle_chromaprint.so"))
    vp, i32 = C.c_void_p, C.c_int
    L.chromaprint_new.restype = vp
    L.chromaprint_new.argtypes = [i32]
    for fn in ("chromaprint_free", "chromaprint_dealloc"):
        getattr(L, fn).argtypes = [vp]
        getattr(L, fn).restype = None
    L.chromaprint_start.argtypes = [vp, i32, i32]
    L.chromaprint_feed.argtypes = [vp, vp, i32]
    L.chromaprint_finish.argtypes = [vp]
    L.chromaprint_clear_fingerprint.argtypes = [vp]
    L.chromaprint_get_fingerprint.argtypes = [vp, C.POINTER(vp)]
    L.chromaprint_get_fingerprint_hash.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.chromaprint_get_raw_fingerprint.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(i32)]
    L.chromaprint_encode_fingerprint.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(i32), i32]
    L.chromaprint_decode_fingerprint.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), i32]
    L.chromaprint_hash_fingerprint.argtypes = [vp, i32, C.POINTER(C.c_uint32)]
    return L


def _encode(L, items, algorithm, base64):
    arr = np.ascontiguousarray(items, dtype=np.uint32)
    out, size = C.c_void_p(), C.c_int(-1)
    assert L.chromaprint_encode_fingerprint(arr.ctypes.data if arr.size else None, arr.size, algorithm, C.byref(out), C.byref(size), base64) == 1
    data = C.string_at(out, size.value)
    assert C.string_at(out, size.value + 1)[-1] == 0                         # NUL-terminated either way
    L.chromaprint_dealloc(out)
    return data


def _decode(L, data, base64):
    """(items, algorithm), or None where the call returns 0"""
    out, size, algorithm = C.c_void_p(), C.c_int(-1), C.c_int(-1)
    if L.chromaprint_decode_fingerprint(data, len(data), C.byref(out), C.byref(size), C.byref(algorithm), base64) != 1:
        return None
    items = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint32)), (size.value,)).tolist() if size.value else []
    L.chromaprint_dealloc(out)
    return items, algorithm.value


# ---- end to end: upstream's Test2SilenceFp ---------------------------------------------------------------------------------
def test_silence_through_the_libchromaprint_calls():
    L = _chromaprint()
    ctx = L.chromaprint_new(1)
    text, h = C.c_void_p(), C.c_uint32(1)
    assert L.chromaprint_start(ctx, 44100, 1) == 1
    zeros = np.zeros(1024, np.int16)
    for _ in range(130):
        assert L.chromaprint_feed(ctx, zeros.ctypes.data, 1024) == 1
    assert L.chromaprint_get_fingerprint(ctx, C.byref(text)) == 0            # before finish
    assert L.chromaprint_get_fingerprint_hash(ctx, C.byref(h)) == 0
    assert L.chromaprint_finish(ctx) == 1
    assert L.chromaprint_get_fingerprint(ctx, C.byref(text)) == 1
    got = C.string_at(text).decode()
    L.chromaprint_dealloc(text)
    assert got == M.SILENCE_TEXT == "AQAAA0mUaEkSRZEGAA"
    assert L.chromaprint_get_fingerprint_hash(ctx, C.byref(h)) == 1 and h.value == 627964279
    assert L.chromaprint_clear_fingerprint(ctx) == 1
    assert L.chromaprint_get_fingerprint(ctx, C.byref(text)) == 0            # after clear_fingerprint
    L.chromaprint_free(ctx)


# ---- the ten vectors ----------------------------------------------------------------------------------------------------------
def test_the_ten_vectors_both_ways_binary_and_base64():
    L = _chromaprint()
    vectors = M.VECTORS + [(M.SILENCE_ITEMS, M.SILENCE_ALGORITHM, list(M.b64decode(M.SILENCE_TEXT)))]
    assert len(vectors) == 10
    for items, algorithm, want in vectors:
        assert list(_encode(L, items, algorithm, 0)) == want, items
        assert _encode(L, items, algorithm, 1).decode() == M.b64encode(bytes(want))
        assert _decode(L, bytes(want), 0) == (items, algorithm)
        assert _decode(L, M.b64encode(bytes(want)).encode(), 1) == (items, algorithm)
    assert _encode(L, M.SILENCE_ITEMS, 1, 1).decode() == M.SILENCE_TEXT
    assert _encode(L, [1, 2, 3], 0x1234, 0)[0] == 0x34                       # any algorithm byte: a label
    assert _decode(L, bytes([0, 0, 0]), 0) is None and _decode(L, b"A", 1) is None and _decode(L, b"AA+A", 1) is None
    assert _decode(L, bytes([0, 0, 0, 1, 15, 0, 25]), 0) is None             # a bit position of 33
    # the batched calls give the same
    assert [list(b) for b in capi.compress_fingerprints([v[0] for v in M.VECTORS], algorithm=0)] == [v[2] for v in M.VECTORS]
    assert capi.compress_fingerprints([M.SILENCE_ITEMS], base64=True) == [M.SILENCE_TEXT]
    arrays, algorithms, status = capi.decompress_fingerprints([M.SILENCE_TEXT], base64=True)
    assert arrays[0].tolist() == M.SILENCE_ITEMS and algorithms == [1] and status == [0]
    assert capi.compress_fingerprints([]) == [] and capi.decompress_fingerprints([]) == ([], [], [])


# ---- edges of the compress tile -------------------------------------------------------------------------------------------
def _contents(n, kind, rng):
    """items whose deltas are of one kind"""
    if kind == "zero":
        x = np.zeros(n, np.uint32)
    elif kind == "dense":                                                    # items alternate 0xFFFFFFFF and 0: x all ones
        x = np.full(n, 0xFFFFFFFF, np.uint32)
    elif kind == "bit31":
        x = np.full(n, 1 << 31, np.uint32)
    elif kind == "gap6_gap7":                                                # bits 0 and 6 against bits 0 and 7
        x = np.where(np.arange(n) % 2 == 0, 0x41, 0x81).astype(np.uint32)
    elif kind == "bits0_31":
        x = np.full(n, 0x80000001, np.uint32)
    else:                                                                    # 0 to 8 random bits
        x = np.zeros(n, np.uint32)
        for i in range(n):
            for b in rng.integers(0, 32, rng.integers(0, 9)):
                x[i] |= np.uint32(1) << np.uint32(b)
    return np.bitwise_xor.accumulate(x) if n else x


def test_edges_of_the_compress_tile_in_one_batch():
    T, _ = capi.fingerprint_codec_tiles()
    rng = np.random.default_rng(3)
    fps = []
    for kind in ("zero", "dense", "bit31", "gap6_gap7", "bits0_31", "random"):
        for n in (0, 1, 2, T - 1, T, T + 1, 3 * T + 5):
            fps.append(_contents(n, kind, rng))
        fps.append(np.zeros(0, np.uint32))                                   # empty fingerprints between the kinds
    want = [M.compress(f.tolist(), 1) for f in fps]
    got = capi.compress_fingerprints(fps, algorithm=1)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"fingerprint {b} ({len(fps[b])} items): bytes differ from the model's"
        assert len(g) <= capi.fingerprint_compressed_bound(len(fps[b]))
    arrays, algorithms, status = capi.decompress_fingerprints(want)
    assert status == [0] * len(fps) and algorithms == [1] * len(fps)
    for b, (a, f) in enumerate(zip(arrays, fps)):
        assert np.array_equal(a, f), f"fingerprint {b} ({len(f)} items): items differ after the round trip"


# ---- edges of the decompress tile -----------------------------------------------------------------------------------------
def test_edges_of_the_decompress_tile():
    _, D = capi.fingerprint_codec_tiles()
    rng = np.random.default_rng(4)
    fps = [np.zeros(n, np.uint32) for n in (D - 1, D, D + 1)]                 # exactly that many symbols
    dense = _contents(2 * D // 33 + 40, "dense", rng)                         # 33 symbols an item: more than two tiles' worth
    assert 2 * D < 33 * len(dense) <= 3 * D
    fps += [dense, _contents(D, "random", rng)]
    blobs = [M.compress(f.tolist(), 1) for f in fps]
    for f, n in zip(fps[:3], (D - 1, D, D + 1)):
        assert len(M.symbols(f.tolist())[0]) == n
    arrays, algorithms, status = capi.decompress_fingerprints(blobs)
    assert status == [0] * len(fps)
    for a, f in zip(arrays, fps):
        assert np.array_equal(a, f)
    assert capi.compress_fingerprints(fps) == blobs


# ---- refusals, beside good blobs --------------------------------------------------------------------------------------------
def test_refusals_in_one_batch_with_good_neighbours():
    good = [M.compress([0x80000001, 1 << 8, 7], 1), M.compress(list(range(1, 200)), 2)]
    blob = good[0]
    blobs = [good[1]]
    blobs += [blob[:k] for k in range(len(blob))]                            # every truncation
    blobs += [good[0]]
    blobs += [bytes([0, 0xFF, 0xFF, 0xFF]),                                  # n = 2^24 - 1 on four bytes
              bytes([0, 0, 0, 3, 0]),                                        # n above floor(8 (L - 4) / 3)
              bytes([0, 0, 0, 1, 15, 0, 25]),                                # gaps 32 + 1: position 33
              good[1],
              blob + bytes(range(240, 256)),                                 # trailing garbage
              bytes([5, 0, 0, 0, 0xAB]),                                     # n = 0 and a byte behind the header
              good[0]]
    want = [M.decompress(b) for b in blobs]
    arrays, algorithms, status = capi.decompress_fingerprints(blobs)
    assert status == [w[2] for w in want]
    assert set(status) == {0, 1, 2, 3, 4}
    assert algorithms == [w[1] for w in want]
    for b, (a, w) in enumerate(zip(arrays, want)):
        assert a.tolist() == w[0], f"blob {b}"
        assert w[2] == 0 or len(a) == 0                                      # a refused blob's slot is empty
    assert arrays[0].tolist() == list(range(1, 200)) and arrays[-1].tolist() == [0x80000001, 1 << 8, 7]
    assert arrays[-3].tolist() == [0x80000001, 1 << 8, 7] and status[-3] == 0  # trailing bytes are ignored


# ---- a feeder's lanes -----------------------------------------------------------------------------------------------------------
FEEDER_KERNELS = ("stft_chroma32", "stft_chroma", "features_cert", "stft_fallback", "fixup_items", "features_classify", "fir_norm",
                  "classify", "feeder_carry", "resample", "ingest", "convert", "downmix", "rematrix")
CODEC_KERNELS = ("fp_compress_count", "fp_compress_layout", "fp_compress_zero", "fp_compress_pack")


def _tonal(seconds, f0, rate=11025):
    t = np.arange(int(seconds * rate)) / rate
    return (9000 * np.sin(2 * np.pi * f0 * t * (1 + 0.3 * np.sin(2 * np.pi * 0.7 * t))) + 3000 * np.sin(2 * np.pi * 3.1 * f0 * t)).astype(np.int16)


def _run_feeder(streams, cuts, ask):
    """Feeds two lanes in ragged chunks; `ask`: also call compressed() on the way.  -> (items, blobs or None, launches)"""
    capi.set_kernel_timing("all,sum")
    try:
        f = capi.Feeder(2, 1, 11025, capi.SAMPLE_S16, 1)
        at = [0, 0]
        for step in cuts:
            chunk = [s[a: a + c] for s, a, c in zip(streams, at, step)]
            at = [a + c for a, c in zip(at, step)]
            f.feed(chunk)
            if ask:
                with pytest.raises(capi.NeedleError, match="InvalidArgument"):
                    f.compressed(0)                                          # an unfinished lane
        f.feed([s[a:] for s, a in zip(streams, at)])
        f.finish([1])
        blobs = None
        if ask:
            with pytest.raises(capi.NeedleError, match="InvalidArgument"):
                f.compressed(0)
            one = f.compressed(1)
        f.finish()
        if ask:
            blobs = [f.compressed(0), f.compressed(1), f.compressed(1, algorithm=3, base64=True)]
            assert blobs[1] == one
            with pytest.raises(capi.NeedleError, match="InvalidArgument"):
                f.compressed(2)
        items = [f.items(0), f.items(1)]
        capi.synchronize()
        launches = {k: capi.kernel_launches(k) for k in FEEDER_KERNELS + CODEC_KERNELS}
        return items, blobs, launches
    finally:
        capi.set_kernel_timing(None)


def test_a_feeders_lanes_compressed_and_the_feeder_untouched():
    streams = [_tonal(9.0, 440.0), _tonal(6.5, 523.0)]
    cuts = [(3001, 17000), (20000, 1), (12345, 30000), (7, 4096)]
    items, blobs, launches = _run_feeder(streams, cuts, True)
    assert len(items[0]) > 40 and len(items[1]) > 25
    assert blobs[0] == M.compress(items[0].tolist(), 1) and blobs[1] == M.compress(items[1].tolist(), 1)
    assert blobs[2] == M.b64encode(M.compress(items[1].tolist(), 3))
    assert all(launches[k] == 4 for k in CODEC_KERNELS)                      # four successful calls, one chain each
    twin_items, _, twin_launches = _run_feeder(streams, cuts, False)
    assert all(np.array_equal(a, b) for a, b in zip(items, twin_items))
    assert all(twin_launches[k] == 0 for k in CODEC_KERNELS)
    assert {k: launches[k] for k in FEEDER_KERNELS} == {k: twin_launches[k] for k in FEEDER_KERNELS}
    assert sum(twin_launches[k] for k in FEEDER_KERNELS) > 0


# ---- the hash -------------------------------------------------------------------------------------------------------------------
def test_hash_is_the_oracles_simhash():
    L = _chromaprint()
    rng = np.random.default_rng(9)
    for n in (0, 1, 2, 63, 64, 65, 1000):
        fp = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        h = C.c_uint32(0xDEADBEEF)
        assert L.chromaprint_hash_fingerprint(fp.ctypes.data if n else None, n, C.byref(h)) == 1
        assert h.value == O.simhash32(fp.tolist())
    assert h.value is not None and O.simhash32([]) == 0
