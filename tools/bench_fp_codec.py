"""Cost of chromaprint's fingerprint codec on the device (needle_hip_fingerprint_compress_host / _decompress_host): prints
one JSON line and writes it to --out.

  workload : --fingerprints (2000) fingerprints of --items (21 764: a 45-minute episode at the default step) items whose
             deltas have 0 to 8 random bits, compressed in one call and decompressed in one call.
  kernels  : every kernel of both launch chains by the library's event timers ("sum" mode: all launches of a name since
             the selection, so a call that is cut into batches counts whole), the median over --steps calls after --warmup.
  bytes    : items in (4 B each) and blob bytes out for compress, the reverse for decompress; GB/s = (in + out) / kernel time.
  wall     : the whole call from host arrays to host arrays: uploads, allocations, the kernels, downloads.
  yardstick: the plain sequential codec of tests/cpp/fp_codec_check.cpp, built -O2, on one core of the same machine, over
             the same shape (its own random deltas of the same distribution).  Host code that is not under test; the ratio
             is written down, not asserted.

Usage: python tools/bench_fp_codec.py [--fingerprints N] [--items K] [--steps S] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from needle_amd import capi  # noqa: E402

COMPRESS = ("fp_compress_count", "fp_compress_layout", "fp_compress_zero", "fp_compress_pack")
DECOMPRESS = ("fp_decompress_count", "fp_decompress_layout", "fp_decompress_unpack", "fp_decompress_xor")


def random_fingerprints(count, items, seed=1):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 9, (count, items))
    x = np.zeros((count, items), np.uint32)
    for k in range(8):
        x |= np.where(bits > k, np.uint32(1) << rng.integers(0, 32, (count, items)).astype(np.uint32), np.uint32(0)).astype(np.uint32)
    return np.bitwise_xor.accumulate(x, axis=1)


def timed(names, call, steps, warmup):
    kernel = {k: [] for k in names}
    wall = []
    result = None
    for step in range(warmup + steps):
        capi.set_kernel_timing(",".join(names) + ",sum")
        t0 = time.perf_counter()
        result = call()
        t1 = time.perf_counter()
        capi.synchronize()
        if step >= warmup:
            wall.append((t1 - t0) * 1e3)
            for k in names:
                kernel[k].append(capi.last_kernel_ms(k))
    capi.set_kernel_timing(None)
    ms = {k: statistics.median(v) for k, v in kernel.items()}
    return result, ms, statistics.median(wall)


def yardstick(count, items):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "fp_codec_check")
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "needle_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "fp_codec_check.cpp")], check=True)
        out = subprocess.run(["taskset", "-c", "0", exe, "bench", str(count), str(items)], capture_output=True, text=True)
        if out.returncode != 0:  # no taskset, or CPU 0 is not ours: one thread all the same
            out = subprocess.run([exe, "bench", str(count), str(items)], capture_output=True, text=True, check=True)
        return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fingerprints", type=int, default=2000)
    ap.add_argument("--items", type=int, default=21764)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp_codec_bench.json"))
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_fp_codec needs a HIP device: the codec has no CPU path")
    fps = random_fingerprints(a.fingerprints, a.items)
    rows = [fps[b] for b in range(a.fingerprints)]
    blobs, c_ms, c_wall = timed(COMPRESS, lambda: capi.compress_fingerprints(rows), a.steps, a.warmup)
    (arrays, _, status), d_ms, d_wall = timed(DECOMPRESS, lambda: capi.decompress_fingerprints(blobs), a.steps, a.warmup)
    assert status == [0] * a.fingerprints and all(np.array_equal(x, y) for x, y in zip(arrays, rows)), "round trip"
    item_bytes, blob_bytes = 4 * fps.size, sum(len(b) for b in blobs)
    c_total, d_total = sum(c_ms.values()), sum(d_ms.values())
    ref = yardstick(a.fingerprints, a.items)
    res = {
        "workload": {"fingerprints": a.fingerprints, "items_each": a.items, "deltas": "0 to 8 random bits", "steps": a.steps, "warmup": a.warmup},
        "bytes": {"items": item_bytes, "blobs": blob_bytes, "blob_bytes_per_item": blob_bytes / fps.size},
        "compress": {"kernel_ms": c_ms, "kernel_ms_total": c_total, "gb_per_s": (item_bytes + blob_bytes) / c_total / 1e6, "call_wall_ms": c_wall},
        "decompress": {"kernel_ms": d_ms, "kernel_ms_total": d_total, "gb_per_s": (item_bytes + blob_bytes) / d_total / 1e6, "call_wall_ms": d_wall},
        "yardstick_one_core": {"compress_ms": ref["compress_s"] * 1e3, "decompress_ms": ref["decompress_s"] * 1e3, "blob_bytes": ref["blob_bytes"]},
        "ratio_yardstick_over_kernels": {"compress": ref["compress_s"] * 1e3 / c_total, "decompress": ref["decompress_s"] * 1e3 / d_total},
        "ratio_yardstick_over_call_wall": {"compress": ref["compress_s"] * 1e3 / c_wall, "decompress": ref["decompress_s"] * 1e3 / d_wall},
        "measured": "kernel_ms, call_wall_ms, bytes, yardstick",
        "derived": "gb_per_s, the ratios",
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
