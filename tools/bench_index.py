"""Cost of growing a library with the incremental index (needle_hip_index_*): prints one JSON document.

For N = 250, 500 and 1000 videos of 45 minutes (synthetic tonal episodes generated on the device, synth.DeviceLibrary, the
default opening window of 50 %, analyzed once and reused):
  append_1 / append_8   : wall time of needle_hip_index_add of 1 / 8 new videos to an index holding N
  full_1 / full_8       : wall time of needle_hip_comparator_run_with_frame_hashes over the same N + 1 / N + 8 videos
  kernels               : event-timed kernel milliseconds of one such call (scan = hamming_runs + simhash_runs; the index's
                          entries = index_buckets + index_entries, its best match = index_best_match; the full search's
                          epilogue_buckets + epilogue_entries and epilogue_best_match), from a separate pass with timing on
Medians over --steps calls after --warmup.

Usage: python tools/bench_index.py [--sizes 250,500,1000] [--steps K] [--warmup W] [--out profiles/index_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from needle_amd import capi, synth  # noqa: E402

EPISODE_S = 45 * 60
WINDOW = int(EPISODE_S * capi.DEFAULT_OPENING_SEARCH_PERCENTAGE * synth.RATE)
SCAN = ("hamming_runs", "hamming_runs_unstaged", "simhash_runs")
INDEX = ("index_buckets", "index_entries", "index_best_match")
FULL = ("epilogue_buckets", "epilogue_entries", "epilogue_best_match")


def analyze(count, chunk=256):
    """count videos' opening windows, generated and fingerprinted on the device in chunks."""
    out = []
    for first in range(0, count, chunk):
        n = min(chunk, count - first)
        gen = synth.DeviceLibrary(n, WINDOW, 60.0, first_episode=first)
        lib = capi.Library(n, opening_search_percentage=1.0)
        lib.set_pcm_device(gen.pointers(), [WINDOW] * n)
        lib.analyze()
        out += [lib.frame_hashes(v) for v in range(n)]
        gen.free()
        del lib
    return out


def comparator(n):
    return capi.Comparator([f"ep{k:04d}.mkv" for k in range(max(n, 2))])


def kernel_ms(names):
    return {k: round(v, 4) for k in names for v in [capi.last_kernel_ms(k)] if v >= 0}


def timed(fn):
    capi.synchronize()
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def bench(fhs, n, k, steps, warmup):
    out = {}
    # the index: a fresh one holding n per measurement, then the append of k
    appends = []
    for rep in range(warmup + steps):
        index = capi.Index(comparator(n))
        index.add(fhs[:n])
        ms = timed(lambda: index.add(fhs[n:n + k]))
        assert index.pairs_searched()[1] == n * k + k * (k - 1) // 2
        if rep >= warmup:
            appends.append(ms)
        del index
    full = []
    cmp = comparator(n + k)
    for rep in range(warmup + steps):
        ms = timed(lambda: cmp.run_with_frame_hashes(fhs[:n + k]))
        if rep >= warmup:
            full.append(ms)
    # kernel times: one more call of each with the event timers on ("sum": every launch of the call adds up)
    index = capi.Index(comparator(n))
    index.add(fhs[:n])
    capi.set_kernel_timing(",".join(SCAN + INDEX) + ",sum")
    index.add(fhs[n:n + k])
    idx_k = kernel_ms(SCAN + INDEX)
    same = cmp.run_with_frame_hashes(fhs[:n + k])
    assert [None if r is None else (r.opening, r.ending) for r in same] == \
        [None if r is None else (r.opening, r.ending) for r in index.results()], "index and full search disagree"
    capi.set_kernel_timing(",".join(SCAN + FULL) + ",sum")
    cmp.run_with_frame_hashes(fhs[:n + k])
    full_k = kernel_ms(SCAN + FULL)
    capi.set_kernel_timing(None)
    out[f"append_{k}_ms"] = round(statistics.median(appends), 3)
    out[f"full_{k}_ms"] = round(statistics.median(full), 3)
    out[f"speedup_{k}"] = round(statistics.median(full) / statistics.median(appends), 2)
    out[f"append_{k}_kernels_ms"] = idx_k
    out[f"full_{k}_kernels_ms"] = full_k
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="250,500,1000")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_index.py needs a HIP device")
    sizes = [int(x) for x in a.sizes.split(",")]
    t = time.perf_counter()
    fhs = analyze(max(sizes) + 8)
    doc = {"machine": "AMD Instinct MI355X (gfx950), one GPU", "device": capi.device_pci_bus_id(), "episode_s": EPISODE_S, "window_hashes": len(fhs[0].opening_data()[0]),
           "analyze_s": round(time.perf_counter() - t, 1), "steps": a.steps, "warmup": a.warmup, "sizes": {}}
    for n in sizes:
        row = {}
        for k in (1, 8):
            row.update(bench(fhs, n, k, a.steps, a.warmup))
        doc["sizes"][str(n)] = row
        print(json.dumps({str(n): row}), file=sys.stderr, flush=True)
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
