#!/usr/bin/env python3
"""What a feed of the streaming comparator (needle_hip_matcher_*) costs -> profiles/matcher_bench.json.

  per_feed : ms per feed of one-second chunks (4 kept items at step 2) for 1, 28 and 256 lanes x 250 and 1 000 sources of
             5 441 hashes (the 45-minute opening windows of tools/bench_index.py's episodes): wall time (median of 50 feeds
             after 20 untimed) and, in a pass of its own, the three kernels' event time (mean over 50 feeds).
  prefix   : 1 lane x 1 000 sources at prefix lengths of 1, 10 and 40 minutes, five repetitions of the 50-feed median each,
             next to the yardstick -- what a caller does without the matcher: needle_hip_hamming_runs_host over the whole
             prefix after each feed, in a fresh process on the parent commit's library (--parent; this tree's without).
             ASSERTED: the 40-minute median lies within the run-to-run
             spread (max - min of the five repetitions) of the 1-minute median.  The ratio to the yardstick is recorded,
             it is no target.
  cell_rate: one feed of a whole 5 441-item lane against 1 000 sources, the strip kernel's cells per second as a share of
             needle_hip_int_valu_ceiling(), next to hamming_runs_kernel<true> (NEEDLE_HIP_GENERIC_SEARCH=1,
             NEEDLE_HIP_SCAN_MFMA=0) on the same pairs.
  resources: registers, LDS and scratch of the matcher's kernels and of every kernel of search.hip and the fingerprint
             files, from the compiler's remarks, for this tree and (--parent) for a checkout of the parent commit.
  headline : bench.py --gpus 1 --steps 20 --warmup 5, parent and this tree alternating, four runs each (--parent, built; --repeats).

Sections that were not run keep what the file held, or "not measured".

usage: python tools/bench_matcher.py [--only per_feed,prefix,cell_rate,resources,headline] [--parent DIR]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NOT_MEASURED = "not measured"
SOURCE_LEN, CHUNK, THRESHOLD, MIN_LEN = 5441, 4, 10, 80    # min_len: 20 s of 0.2477 s items
KERNELS = ("matcher_land", "matcher_strip", "matcher_simhash")


def sources_and_lane(num_sources, lane_items, seed=7):
    """Unrelated hashes with one shared opening of 360 items (90 s) in every source and in the lane."""
    rng = np.random.default_rng(seed)
    opening = rng.integers(0, 2 ** 32, 360, dtype=np.uint64).astype(np.uint32)
    srcs = rng.integers(0, 2 ** 32, (num_sources, SOURCE_LEN), dtype=np.uint64).astype(np.uint32)
    for k in range(num_sources):
        at = 100 + 37 * (k % 50)
        srcs[k, at:at + 360] = opening ^ (np.uint32(1) << rng.integers(0, 32, 360).astype(np.uint32))
    lane = rng.integers(0, 2 ** 32, lane_items, dtype=np.uint64).astype(np.uint32)
    if lane_items >= 700:
        lane[300:660] = opening
    return list(srcs), lane


def timed_feeds(capi, m, lanes, chunks, count):
    out = []
    for _ in range(count):
        feed = [next(chunks) for _ in range(lanes)]
        t0 = time.perf_counter()
        m.feed(feed)
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def chunk_source(seed):
    rng = np.random.default_rng(seed)
    while True:
        block = rng.integers(0, 2 ** 32, (4096, CHUNK), dtype=np.uint64).astype(np.uint32)
        for row in block:
            yield row


def bench_per_feed(capi):
    res = {}
    for num_sources in (250, 1000):
        srcs, _ = sources_and_lane(num_sources, 0)
        for lanes in (1, 28, 256):
            m = capi.Matcher(srcs, [MIN_LEN] * num_sources, lanes, THRESHOLD)
            chunks = chunk_source(lanes)
            timed_feeds(capi, m, lanes, chunks, 20)
            wall = timed_feeds(capi, m, lanes, chunks, 50)
            capi.set_kernel_timing(",".join(KERNELS) + ",sum")
            timed_feeds(capi, m, lanes, chunks, 50)
            capi.synchronize()
            kernels = {k: round(capi.last_kernel_ms(k) / 50, 5) for k in KERNELS}
            capi.set_kernel_timing(None)
            feeds, launches, cells, state = m.stats()
            res[f"{lanes} lanes x {num_sources} sources"] = {
                "wall_ms_per_feed_median": round(statistics.median(wall), 5), "wall_ms_min_max": [round(min(wall), 5), round(max(wall), 5)],
                "kernel_ms_per_feed_mean": kernels, "kernel_ms_per_feed_sum": round(sum(kernels.values()), 5),
                "cells_per_feed": cells // feeds, "launches_per_feed": launches // feeds, "state_bytes": state}
            print("per_feed", lanes, num_sources, res[f"{lanes} lanes x {num_sources} sources"], file=sys.stderr, flush=True)
            del m
    return res


_YARDSTICK_CHILD = """
import json, sys, time
import numpy as np
from needle_amd import capi
data = np.load(sys.argv[1])
srcs, lane = list(data["srcs"]), data["lane"]
problems = [(q, len(srcs), int(sys.argv[2])) for q in range(len(srcs))]
out = {}
for items in json.loads(sys.argv[4]):
    seqs = [*srcs, lane[:items]]
    capi.hamming_runs(seqs, problems, int(sys.argv[3]))
    ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        capi.hamming_runs(seqs, problems, int(sys.argv[3]))
        ms.append((time.perf_counter() - t0) * 1e3)
    out[str(items)] = ms
print(json.dumps(out))
"""


def yardstick(tree, srcs, lane, prefixes):
    """needle_hip_hamming_runs_host over the whole prefix, wall ms of five calls per prefix length, in a fresh process that
    loads `tree`'s package and library."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "seqs.npz")
        np.savez(path, srcs=np.stack(srcs), lane=lane)
        env = dict(os.environ, PYTHONPATH=tree)
        run = subprocess.run([sys.executable, "-c", _YARDSTICK_CHILD, path, str(MIN_LEN), str(THRESHOLD), json.dumps(prefixes)], cwd=tree, env=env,
                             stdout=subprocess.PIPE, text=True, timeout=600, check=True)
    return {int(k): v for k, v in json.loads(run.stdout.strip().splitlines()[-1]).items()}


def bench_prefix(capi, parent):
    num_sources = 1000
    srcs, lane = sources_and_lane(num_sources, 9600 + 5 * 70 * CHUNK + 64)
    minutes = {1: 240, 10: 2400, 40: 9600}                                       # items: 4 a second
    res = {"sources": num_sources, "lanes": 1, "chunk_items": CHUNK,
           "yardstick_library": "the parent commit's" if parent else "this tree's (no --parent; the entry point's code is the parent's)",
           "matcher": {}, "yardstick": {}}
    yard_ms = yardstick(parent or ROOT, srcs, lane, list(minutes.values()))
    reps = {label: [] for label in minutes}
    for rep in range(5):                                                         # the prefix lengths alternate: drift is not prefix
        for label, items in minutes.items():
            m = capi.Matcher(srcs, [MIN_LEN] * num_sources, 1, THRESHOLD)
            at = items + rep * 70 * CHUNK                                        # (another stretch of the lane every time)
            m.feed([lane[:at]])
            chunks = iter([lane[at + k * CHUNK: at + (k + 1) * CHUNK] for k in range(70)])
            timed_feeds(capi, m, 1, chunks, 20)
            reps[label].append(statistics.median(timed_feeds(capi, m, 1, chunks, 50)))
            del m
    for label, items in minutes.items():
        yard, mine = yard_ms[items], reps[label]
        res["matcher"][f"{label} min"] = {"prefix_items": items, "ms_per_feed_median_of_50": [round(x, 5) for x in mine],
                                          "median": round(statistics.median(mine), 5), "spread": round(max(mine) - min(mine), 5)}
        res["yardstick"][f"{label} min"] = {"ms_per_rescan": [round(x, 4) for x in yard], "median": round(statistics.median(yard), 4)}
        res[f"ratio_yardstick_to_matcher_{label}_min"] = round(statistics.median(yard) / statistics.median(mine), 2)
        print("prefix", label, res["matcher"][f"{label} min"], res["yardstick"][f"{label} min"], file=sys.stderr, flush=True)
    one, forty = res["matcher"]["1 min"], res["matcher"]["40 min"]
    res["asserted"] = "|median(40 min) - median(1 min)| <= spread(1 min), the spread being max - min of its five repetitions"
    res["holds"] = abs(forty["median"] - one["median"]) <= one["spread"]
    return res


def bench_cell_rate(capi):
    num_sources = 1000
    srcs, lane = sources_and_lane(num_sources, SOURCE_LEN)
    ceiling = capi.int_valu_ceiling()
    m = capi.Matcher(srcs, [MIN_LEN] * num_sources, 1, THRESHOLD)
    m.feed([lane])                                                               # (allocations, first launches)
    m.reset()
    t0 = time.perf_counter()
    m.feed([lane])
    wall = (time.perf_counter() - t0) * 1e3                                      # without event timing
    m.reset()
    capi.set_kernel_timing(",".join(KERNELS) + ",sum")
    m.feed([lane])
    capi.synchronize()
    strip_ms = capi.last_kernel_ms("matcher_strip")
    all_ms = {k: round(capi.last_kernel_ms(k), 4) for k in KERNELS}
    capi.set_kernel_timing(None)
    cells = num_sources * (SOURCE_LEN - 1) * (SOURCE_LEN - 1)
    res = {"cells": cells, "int_valu_ceiling_cells_per_s": ceiling,
           "matcher": {"strip_kernel_ms": round(strip_ms, 4), "kernels_ms": all_ms, "wall_ms": round(wall, 3), "rounds": -(-SOURCE_LEN // 512),
                       "cells_per_s": cells / (strip_ms * 1e-3), "share_of_ceiling": round(cells / (strip_ms * 1e-3) / ceiling, 4)}}
    old = {k: os.environ.get(k) for k in ("NEEDLE_HIP_GENERIC_SEARCH", "NEEDLE_HIP_SCAN_MFMA")}
    os.environ["NEEDLE_HIP_GENERIC_SEARCH"], os.environ["NEEDLE_HIP_SCAN_MFMA"] = "1", "0"
    try:
        problems = [(q, num_sources, MIN_LEN) for q in range(num_sources)]
        seqs = [*srcs, lane]
        capi.hamming_runs(seqs, problems, THRESHOLD)
        capi.set_kernel_timing("hamming_runs,sum")
        capi.hamming_runs(seqs, problems, THRESHOLD)
        capi.synchronize()
        generic_ms = capi.last_kernel_ms("hamming_runs")
        capi.set_kernel_timing(None)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    res["generic_hamming_runs_kernel"] = {"kernel_ms": round(generic_ms, 4), "cells_per_s": cells / (generic_ms * 1e-3),
                                          "share_of_ceiling": round(cells / (generic_ms * 1e-3) / ceiling, 4)}
    res["strip_over_generic_time"] = round(strip_ms / generic_ms, 3)
    return res


RESOURCE_FILES = ["matcher.hip", "search.hip", "fingerprint.hip", "fingerprint32.hip", "feeder.hip"]
RESOURCE_KEYS = {"TotalSGPRs": "sgprs", "SGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
                 "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}


def kernel_resources(root):
    """{kernel: {sgprs, vgprs, agprs, scratch, occupancy, lds}} of a tree, compiled for gfx950 with the Makefile's flags
    (device side only, nothing is written)."""
    csrc = os.path.join(root, "needle_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out, mangled = {}, []
    for name in RESOURCE_FILES:
        if not os.path.exists(os.path.join(csrc, name)):
            continue
        cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I../../include", "--offload-arch=gfx950", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", "-c", name, "-o", os.devnull]
        if name == "fingerprint32.hip":
            cmd.insert(1, "-fno-slp-vectorize")
        text = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
        cur = None
        for m in re.finditer(r"remark:\s+(.+?): (\S+) \[-Rpass-analysis", text):
            key, val = m.group(1), m.group(2)
            if key == "Function Name":
                cur = out.setdefault(val, {})
                mangled.append(val)
            elif cur is not None and key in RESOURCE_KEYS:
                cur[RESOURCE_KEYS[key]] = int(val)
    plain = subprocess.run(["c++filt", "-p"], input="\n".join(mangled), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    names = {m: p.replace("needle::(anonymous namespace)::", "").replace("needle::", "").replace("void ", "") for m, p in zip(mangled, plain)}
    return {names[m]: v for m, v in out.items()}


def bench_resources(root, parent):
    this = kernel_resources(root)
    new = {k: v for k, v in sorted(this.items()) if k.startswith("matcher_")}
    res = {"how": "hipcc -Rpass-analysis=kernel-resource-usage, gfx950, the Makefile's flags", "matcher_kernels": new}
    if parent:
        before = kernel_resources(parent)
        shared = sorted(set(this) & set(before))
        res["existing_kernels_compared"] = len(shared)
        res["existing_kernels_unchanged"] = all(this[k] == before[k] for k in shared)
        res["changed"] = {k: {"this": this[k], "parent": before[k]} for k in shared if this[k] != before[k]}
        res["gone"] = sorted(set(before) - set(this))
        res["new"] = sorted(set(this) - set(before))
    else:
        res["existing_kernels_unchanged"] = NOT_MEASURED
    return res


def bench_headline(root, parent, repeats=4):
    def once(tree):
        run = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree,
                             stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=600, check=True)
        return json.loads(run.stdout.strip().splitlines()[-1])["value"]
    values = {"parent": [], "this": []}
    for _ in range(repeats):
        values["parent"].append(once(parent))
        values["this"].append(once(root))
        print("headline", values["parent"][-1], values["this"][-1], file=sys.stderr, flush=True)
    med = {k: statistics.median(v) for k, v in values.items()}
    return {"unit": "bench.py's value", "runs": values, "median": med,
            "this_within_parents_spread": min(values["parent"]) <= med["this"] <= max(values["parent"]) or med["this"] >= med["parent"],
            "difference_percent": round(100.0 * (med["this"] - med["parent"]) / med["parent"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="per_feed,prefix,cell_rate,resources,headline")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, built (yardstick, resources, headline)")
    ap.add_argument("--repeats", type=int, default=4, help="headline runs per tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matcher_bench.json"))
    args = ap.parse_args()
    from needle_amd import capi
    only = set(args.only.split(","))
    keys = ("device", "per_feed", "prefix", "cell_rate", "resources", "headline_vs_parent")
    res = {k: NOT_MEASURED for k in keys}
    if os.path.exists(args.out):
        try:
            res.update({k: v for k, v in json.load(open(args.out)).items() if k in keys})
        except (OSError, ValueError):
            pass

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    if "resources" in only:
        res["resources"] = bench_resources(ROOT, args.parent)
        save()
    holds = True
    if capi.device_count() > 0:
        res["device"] = capi.device_pci_bus_id()
        if "per_feed" in only:
            res["per_feed"] = bench_per_feed(capi)
            save()
        if "cell_rate" in only:
            res["cell_rate"] = bench_cell_rate(capi)
            save()
        if "prefix" in only:
            res["prefix"] = bench_prefix(capi, args.parent)
            holds = res["prefix"]["holds"]
            save()
        if "headline" in only and args.parent:
            res["headline_vs_parent"] = bench_headline(ROOT, args.parent, args.repeats)
    save()
    print(json.dumps(res))
    if not holds:
        sys.exit("the matcher's feed depends on the prefix length: see prefix.matcher")


if __name__ == "__main__":
    main()
