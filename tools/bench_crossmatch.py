#!/usr/bin/env python3
"""What the streaming all-pairs comparator (needle_hip_crossmatcher_*) costs -> profiles/crossmatch_bench.json.

Random hashes with one shared opening of 360 items in every lane, threshold 10, min_len 80, one-second chunks (4 kept
items per lane and feed).

  per_feed : 4 / 28 / 64 lanes, taken when the lanes hold 1 / 10 / 24 minutes (240 / 2 400 / 5 760 items): wall ms per feed
             (median of 30 feeds after 10 untimed) and, in a pass of its own, the three kernels' event time (mean over 30
             feeds), with the cells of a feed beside them.  A feed's cost grows with what the other lanes hold (about
             2 J W cells per pair), unlike the matcher's.
  tail     : time from the last chunk to the complete run list, 28 lanes x 2 897 hashes: the last feed plus the finish
             round, wall ms.  The yardstick is what a caller does without the cross-matcher: needle_hip_hamming_runs_host
             over all 378 pairs after the last chunk, in a process of its own on the parent commit's library (--parent; this
             tree's without).  The two alternate; medians of 5; the ratio is recorded, it is no target.
  season   : the same 28 x 2 897 season fed second by second: the sum of the walk kernel's event times over all feeds, next
             to the one-shot scan of the same pairs in its generic form (NEEDLE_HIP_GENERIC_SEARCH=1, NEEDLE_HIP_SCAN_MFMA=0),
             and both as cells per second against needle_hip_int_valu_ceiling().
  resources: registers, LDS and scratch of the new kernels and of every kernel of matcher.hip, search.hip, the fingerprint
             files and feeder.hip, from the compiler's remarks, for this tree and (--parent) for a checkout of the parent
             commit (tools/bench_matcher.py's reader; needs no GPU).
  regions  : openings and endings in ONE object (needle_hip_crossmatcher_new_regions) against what a caller needed before it,
             two single-region cross-matchers fed in turn on the parent commit's library: 28 videos, openings of 2 897 and
             endings of 1 443 items, taken when the lanes hold 1 100 items, 4 new items per lane and feed.  Wall ms per feed
             (median of 30 after 10; for the two objects a feed is both calls) and, in a pass of its own, the summed event
             times of the kernels (mean of 30); five processes each, alternating.  The condition: one object's median <= the
             yardstick's median + the spread (max - min) of the yardstick's own five.  The ratio is recorded, it is no
             target.  And the single-region path on both trees: regions = 1 at 28 and 64 lanes holding 24 minutes, per-feed
             wall and the walk kernel's event time, this tree and the parent alternating, the one that goes first alternating
             too; the difference of the medians must lie within the parent's own spread.  (--parent, built)
  resident : a new season into a library in ONE object (needle_hip_crossmatcher_new_resident: 1 000 resident videos of 5 441
             hashes, 28 arriving lanes, one region) against what a caller needed before it, one Matcher (1 000 sources, 28
             lanes) plus one CrossMatcher(28) fed in turn on the parent commit's library: taken when the lanes hold 1 100 items,
             4 new items per lane and feed.  Wall ms per feed (median of 30 after 10; for the two objects a feed is both
             calls) and, in a pass of its own, the summed event times of the kernels (mean of 30); five processes each,
             alternating.  The condition is the regions leg's; the ratio and the state bytes are recorded, neither is a
             target.  The single-region, no-resident path on both trees is the regions leg's second half.  (--parent, built)
  headline : bench.py --gpus 1 --steps 20 --warmup 5, parent and this tree alternating, four runs each, the tree that goes
             first alternating too (--parent, built).

Sections that were not run keep what the file held, or "not measured".

usage: python tools/bench_crossmatch.py [--only per_feed,tail,season,resources,regions,resident,headline] [--parent DIR]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_matcher as BM  # noqa: E402  (the compiler-remark reader)

NOT_MEASURED = "not measured"
CHUNK, THRESHOLD, MIN_LEN = 4, 10, 80
SEASON_LANES, SEASON_ITEMS = 28, 2897
KERNELS = ("crossmatch_land", "crossmatch_walk", "crossmatch_simhash")


def season(lanes, items, seed=7):
    """Unrelated hashes with one shared opening of 360 items (90 s), a bit flipped per item, somewhere in every lane's first
    1 900 items."""
    rng = np.random.default_rng(seed)
    opening = rng.integers(0, 2 ** 32, 360, dtype=np.uint64).astype(np.uint32)
    out = rng.integers(0, 2 ** 32, (lanes, items), dtype=np.uint64).astype(np.uint32)
    if items >= 700:
        for k in range(lanes):
            at = 100 + 37 * (k % 40) if items >= 2000 else 100 + 5 * (k % 40)
            out[k, at:at + 360] = opening ^ (np.uint32(1) << rng.integers(0, 32, 360).astype(np.uint32))
    return out


def timed_feeds(m, data, pos, count):
    """`count` feeds of CHUNK items per lane from column `pos` on: (wall ms of each, the next column)."""
    out = []
    for _ in range(count):
        feed = [row[pos: pos + CHUNK] for row in data]
        t0 = time.perf_counter()
        m.feed(feed)
        out.append((time.perf_counter() - t0) * 1e3)
        pos += CHUNK
    return out, pos


def bench_per_feed(capi):
    res = {}
    minutes = {1: 240, 10: 2400, 24: 5760}
    per_level = 70 * CHUNK
    for lanes in (4, 28, 64):
        total = max(minutes.values()) + per_level
        data = season(lanes, total, seed=lanes)
        m = capi.CrossMatcher(lanes, total, MIN_LEN, THRESHOLD)
        pos = 0
        for label, items in minutes.items():
            t0 = time.perf_counter()
            m.feed([row[pos: items] for row in data])                            # up to the level, untimed
            fill_s = time.perf_counter() - t0
            pos = items
            _, pos = timed_feeds(m, data, pos, 10)
            before = m.stats()
            wall, pos = timed_feeds(m, data, pos, 30)
            after = m.stats()
            capi.set_kernel_timing(",".join(KERNELS) + ",sum")
            _, pos = timed_feeds(m, data, pos, 30)
            capi.synchronize()
            kernels = {k: round(capi.last_kernel_ms(k) / 30, 5) for k in KERNELS}
            capi.set_kernel_timing(None)
            key = f"{lanes} lanes at {label} min"
            res[key] = {"items_held": items, "wall_ms_per_feed_median": round(statistics.median(wall), 5),
                        "wall_ms_min_max": [round(min(wall), 5), round(max(wall), 5)],
                        "kernel_ms_per_feed_mean": kernels, "kernel_ms_per_feed_sum": round(sum(kernels.values()), 5),
                        "cells_per_feed": (after[2] - before[2]) // 30, "launches_per_feed": (after[1] - before[1]) // 30,
                        "state_bytes": after[3], "fill_to_level_s": round(fill_s, 3)}
            print("per_feed", key, res[key], file=sys.stderr, flush=True)
        del m
    return res


_YARDSTICK_CHILD = """
import json, sys, time
import numpy as np
from needle_amd import capi
data = np.load(sys.argv[1])["lanes"]
lanes = list(data)
n = len(lanes)
problems = [(a, b, int(sys.argv[2])) for a in range(n) for b in range(a + 1, n)]
capi.hamming_runs(lanes, problems, int(sys.argv[3]))
t0 = time.perf_counter()
runs = capi.hamming_runs(lanes, problems, int(sys.argv[3]))
print(json.dumps({"ms": (time.perf_counter() - t0) * 1e3, "runs": int(len(runs))}))
"""


def bench_tail(capi, parent):
    data = season(SEASON_LANES, SEASON_ITEMS)
    head = SEASON_ITEMS - CHUNK
    res = {"lanes": SEASON_LANES, "items": SEASON_ITEMS, "pairs": SEASON_LANES * (SEASON_LANES - 1) // 2, "chunk_items": CHUNK,
           "yardstick_library": "the parent commit's" if parent else "this tree's (no --parent; the entry point's code is the parent's)"}
    stream_ms, yard_ms = [], []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "lanes.npz")
        np.savez(path, lanes=data)
        tree = parent or ROOT
        for _ in range(5):                                                       # the two alternate
            run = subprocess.run([sys.executable, "-c", _YARDSTICK_CHILD, path, str(MIN_LEN), str(THRESHOLD)], cwd=tree,
                                 env=dict(os.environ, PYTHONPATH=tree), stdout=subprocess.PIPE, text=True, timeout=600, check=True)
            got = json.loads(run.stdout.strip().splitlines()[-1])
            yard_ms.append(got["ms"])
            m = capi.CrossMatcher(SEASON_LANES, SEASON_ITEMS, MIN_LEN, THRESHOLD)
            m.feed([row[:head - CHUNK] for row in data])
            m.feed([row[head - CHUNK: head] for row in data])                    # (a feed of the timed shape before it)
            t0 = time.perf_counter()
            m.feed([row[head:] for row in data])
            m.finish()
            count, complete = m.ready()
            stream_ms.append((time.perf_counter() - t0) * 1e3)
            assert complete and count == got["runs"], (complete, count, got["runs"])
            res["runs"] = count
            del m
    res["streaming_last_feed_plus_finish_ms"] = [round(x, 4) for x in stream_ms]
    res["yardstick_one_shot_ms"] = [round(x, 4) for x in yard_ms]
    res["median_ms"] = {"streaming": round(statistics.median(stream_ms), 4), "yardstick": round(statistics.median(yard_ms), 4)}
    res["ratio_yardstick_to_streaming"] = round(statistics.median(yard_ms) / statistics.median(stream_ms), 2)
    return res


def bench_season(capi):
    data = season(SEASON_LANES, SEASON_ITEMS)
    pairs = SEASON_LANES * (SEASON_LANES - 1) // 2
    cells = pairs * (SEASON_ITEMS - 1) * (SEASON_ITEMS - 1)
    ceiling = capi.int_valu_ceiling()
    m = capi.CrossMatcher(SEASON_LANES, SEASON_ITEMS, MIN_LEN, THRESHOLD)
    capi.set_kernel_timing(",".join(KERNELS) + ",sum")
    t0 = time.perf_counter()
    for pos in range(0, SEASON_ITEMS, CHUNK):
        m.feed([row[pos: pos + CHUNK] for row in data])
    m.finish()
    wall = time.perf_counter() - t0
    capi.synchronize()
    kernels = {k: round(capi.last_kernel_ms(k), 4) for k in KERNELS}
    capi.set_kernel_timing(None)
    feeds, launches, walked, _ = m.stats()
    assert walked == cells, (walked, cells)
    walk_ms = kernels["crossmatch_walk"]
    res = {"lanes": SEASON_LANES, "items": SEASON_ITEMS, "pairs": pairs, "cells": cells, "int_valu_ceiling_cells_per_s": ceiling,
           "streamed": {"feeds": feeds, "launches": launches, "kernel_ms_summed": kernels, "wall_s_with_event_timing": round(wall, 3),
                        "runs": m.ready()[0], "cells_per_s": cells / (walk_ms * 1e-3),
                        "share_of_ceiling": round(cells / (walk_ms * 1e-3) / ceiling, 4)}}
    old = {k: os.environ.get(k) for k in ("NEEDLE_HIP_GENERIC_SEARCH", "NEEDLE_HIP_SCAN_MFMA")}
    os.environ["NEEDLE_HIP_GENERIC_SEARCH"], os.environ["NEEDLE_HIP_SCAN_MFMA"] = "1", "0"
    try:
        lanes = list(data)
        problems = [(a, b, MIN_LEN) for a in range(SEASON_LANES) for b in range(a + 1, SEASON_LANES)]
        capi.hamming_runs(lanes, problems, THRESHOLD)
        capi.set_kernel_timing("hamming_runs,sum")
        capi.hamming_runs(lanes, problems, THRESHOLD)
        capi.synchronize()
        generic_ms = capi.last_kernel_ms("hamming_runs")
        capi.set_kernel_timing(None)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    res["one_shot_generic_hamming_runs_kernel"] = {"kernel_ms": round(generic_ms, 4), "cells_per_s": cells / (generic_ms * 1e-3),
                                                   "share_of_ceiling": round(cells / (generic_ms * 1e-3) / ceiling, 4)}
    res["streamed_over_one_shot_time"] = round(walk_ms / generic_ms, 3)
    return res


_REGIONS_CHILD = """
import json, statistics, sys, time
import numpy as np
from needle_amd import capi
mode, videos, held = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
caps = [int(x) for x in sys.argv[4].split(",")]
chunk, threshold, min_len = 4, 10, 80
kernels = ("crossmatch_land", "crossmatch_walk", "crossmatch_simhash")
rng = np.random.default_rng(7)
data = [rng.integers(0, 2 ** 32, (videos, c), dtype=np.uint64).astype(np.uint32) for c in caps]
for d in data:                                       # one shared stretch of 360 items in every lane of a region
    shared = rng.integers(0, 2 ** 32, 360, dtype=np.uint64).astype(np.uint32)
    for k in range(videos):
        at = 100 + 17 * (k % 40)
        d[k, at:at + 360] = shared ^ (np.uint32(1) << rng.integers(0, 32, 360).astype(np.uint32))
if mode == "one":                                    # one object, lane = video * regions + region
    m = capi.CrossMatcher.with_regions(videos, caps, [min_len] * len(caps), threshold)
    objects = [m]
    def feed(a, b):
        m.feed([data[r][v, a:b] for v in range(videos) for r in range(len(caps))])
else:                                                # one single-region object per region, fed in turn
    objects = [capi.CrossMatcher(videos, c, min_len, threshold) for c in caps]
    def feed(a, b):
        for o, d in zip(objects, data):
            o.feed([row[a:b] for row in d])
def timed(pos, count):
    out = []
    for _ in range(count):
        t0 = time.perf_counter()
        feed(pos, pos + chunk)
        out.append((time.perf_counter() - t0) * 1e3)
        pos += chunk
    return out, pos
feed(0, held)
_, pos = timed(held, 10)
wall, pos = timed(pos, 30)
capi.set_kernel_timing(",".join(kernels) + ",sum")
_, pos = timed(pos, 30)
capi.synchronize()
ms = {k: capi.last_kernel_ms(k) / 30 for k in kernels}
capi.set_kernel_timing(None)
for o in objects:
    o.finish()
print(json.dumps({"wall_ms_per_feed_median": statistics.median(wall), "wall_ms_min_max": [min(wall), max(wall)],
                  "kernel_ms_per_feed": ms, "kernel_ms_per_feed_sum": sum(ms.values()),
                  "launches": sum(o.stats()[1] for o in objects), "runs": sum(o.ready()[0] for o in objects),
                  "state_bytes": sum(o.stats()[3] for o in objects)}))
"""


def bench_regions(root, parent):
    def child(tree, mode, videos, held, caps):
        run = subprocess.run([sys.executable, "-c", _REGIONS_CHILD, mode, str(videos), str(held), ",".join(str(c) for c in caps)], cwd=tree,
                             env=dict(os.environ, PYTHONPATH=tree), stdout=subprocess.PIPE, text=True, timeout=600, check=True)
        return json.loads(run.stdout.strip().splitlines()[-1])

    def summary(runs, key):
        vals = [r[key] if isinstance(key, str) else r[key[0]][key[1]] for r in runs]
        return {"runs": [round(v, 5) for v in vals], "median": round(statistics.median(vals), 5), "spread": round(max(vals) - min(vals), 5)}
    res = {"two_regions_in_one_object": NOT_MEASURED, "single_region_against_parent": NOT_MEASURED}
    caps, held = (SEASON_ITEMS, 1443), 1100
    one, two = [], []
    for _ in range(5):                                                           # the two alternate, the yardstick first
        two.append(child(parent, "two", SEASON_LANES, held, caps))
        one.append(child(root, "one", SEASON_LANES, held, caps))
        print("regions", two[-1]["wall_ms_per_feed_median"], one[-1]["wall_ms_per_feed_median"], file=sys.stderr, flush=True)
    assert all(r["runs"] == one[0]["runs"] for r in one + two), [r["runs"] for r in one + two]
    wall_one, wall_two = summary(one, "wall_ms_per_feed_median"), summary(two, "wall_ms_per_feed_median")
    res["two_regions_in_one_object"] = {
        "videos": SEASON_LANES, "max_items": list(caps), "items_held": held, "chunk_items": 4, "runs": one[0]["runs"],
        "launches_in_the_process": {"one_object": one[0]["launches"], "two_objects": two[0]["launches"]},
        "wall_ms_per_feed": {"one_object": wall_one, "two_objects_on_the_parent": wall_two},
        "kernel_ms_per_feed_sum": {"one_object": summary(one, "kernel_ms_per_feed_sum"), "two_objects_on_the_parent": summary(two, "kernel_ms_per_feed_sum")},
        "walk_kernel_ms_per_feed": {"one_object": summary(one, ("kernel_ms_per_feed", "crossmatch_walk")),
                                    "two_objects_on_the_parent": summary(two, ("kernel_ms_per_feed", "crossmatch_walk"))},
        "condition_one_within_yardstick_plus_its_spread": wall_one["median"] <= wall_two["median"] + wall_two["spread"],
        "ratio_two_objects_to_one": round(wall_two["median"] / wall_one["median"], 3)}
    single = {}
    for lanes in (28, 64):
        this, before = [], []
        for k in range(4):                                                       # which tree goes first alternates
            for name in (("parent", "this") if k % 2 == 0 else ("this", "parent")):
                (before if name == "parent" else this).append(child(parent if name == "parent" else root, "two", lanes, 5760, (5760 + 400,)))
        wall = {"this": summary(this, "wall_ms_per_feed_median"), "parent": summary(before, "wall_ms_per_feed_median")}
        walk = {"this": summary(this, ("kernel_ms_per_feed", "crossmatch_walk")), "parent": summary(before, ("kernel_ms_per_feed", "crossmatch_walk"))}
        single[f"{lanes} lanes at 24 min"] = {
            "wall_ms_per_feed": wall, "walk_kernel_ms_per_feed": walk, "state_bytes": {"this": this[0]["state_bytes"], "parent": before[0]["state_bytes"]},
            "wall_difference_within_parents_spread": abs(wall["this"]["median"] - wall["parent"]["median"]) <= wall["parent"]["spread"],
            "walk_difference_within_parents_spread": abs(walk["this"]["median"] - walk["parent"]["median"]) <= walk["parent"]["spread"]}
        print("regions single", lanes, single[f"{lanes} lanes at 24 min"], file=sys.stderr, flush=True)
    res["single_region_against_parent"] = single
    return res


_RESIDENT_CHILD = """
import json, statistics, sys, time
import numpy as np
from needle_amd import capi
mode, residents, videos, items, held = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
chunk, threshold, min_len = 4, 10, 80
rng = np.random.default_rng(7)
rows = rng.integers(0, 2 ** 32, (residents, items), dtype=np.uint64).astype(np.uint32)
data = rng.integers(0, 2 ** 32, (videos, items), dtype=np.uint64).astype(np.uint32)
shared = rng.integers(0, 2 ** 32, 360, dtype=np.uint64).astype(np.uint32)      # one shared stretch of 360 items in every video
for d in (rows, data):
    for k in range(len(d)):
        at = 100 + 17 * (k % 40)
        d[k, at:at + 360] = shared ^ (np.uint32(1) << rng.integers(0, 32, 360).astype(np.uint32))
if mode == "one":                                    # the residents and the arriving lanes in one object
    m = capi.CrossMatcher.with_resident(list(rows), videos, [items], [min_len], threshold)
    kernels = ("crossmatch_land", "crossmatch_walk", "crossmatch_simhash")
    def feed(a, b):
        m.feed([row[a:b] for row in data])
    def finish():
        m.finish()
        return m.ready()[0], m.stats()[1], m.stats()[3]
else:                                                # old x new in a Matcher, new x new in a CrossMatcher, fed in turn
    old = capi.Matcher(list(rows), [min_len] * residents, videos, threshold)
    new = capi.CrossMatcher(videos, items, min_len, threshold)
    kernels = ("matcher_land", "matcher_strip", "matcher_simhash", "crossmatch_land", "crossmatch_walk", "crossmatch_simhash")
    def feed(a, b):
        chunks = [row[a:b] for row in data]
        old.feed(chunks)
        new.feed(chunks)
    def finish():
        old.finish()
        new.finish()
        return sum(old.ready(k)[0] for k in range(videos)) + new.ready()[0], old.stats()[1] + new.stats()[1], old.stats()[3] + new.stats()[3]
def timed(pos, count):
    out = []
    for _ in range(count):
        t0 = time.perf_counter()
        feed(pos, pos + chunk)
        out.append((time.perf_counter() - t0) * 1e3)
        pos += chunk
    return out, pos
t0 = time.perf_counter()
feed(0, held)
fill = time.perf_counter() - t0
_, pos = timed(held, 10)
wall, pos = timed(pos, 30)
capi.set_kernel_timing(",".join(kernels) + ",sum")
_, pos = timed(pos, 30)
capi.synchronize()
ms = {k: capi.last_kernel_ms(k) / 30 for k in kernels}
capi.set_kernel_timing(None)
runs, launches, state = finish()
print(json.dumps({"wall_ms_per_feed_median": statistics.median(wall), "wall_ms_min_max": [min(wall), max(wall)],
                  "kernel_ms_per_feed": ms, "kernel_ms_per_feed_sum": sum(ms.values()), "fill_to_level_s": fill,
                  "launches": launches, "runs": runs, "state_bytes": state}))
"""


def bench_resident(root, parent, residents=1000, videos=SEASON_LANES, items=5441, held=1100):
    def child(tree, mode):
        run = subprocess.run([sys.executable, "-c", _RESIDENT_CHILD, mode, str(residents), str(videos), str(items), str(held)], cwd=tree,
                             env=dict(os.environ, PYTHONPATH=tree), stdout=subprocess.PIPE, text=True, timeout=900, check=True)
        return json.loads(run.stdout.strip().splitlines()[-1])

    def summary(runs, key):
        vals = [r[key] for r in runs]
        return {"runs": [round(v, 5) for v in vals], "median": round(statistics.median(vals), 5), "spread": round(max(vals) - min(vals), 5)}
    one, parts = [], []
    for _ in range(5):                                                           # the two alternate, the yardstick first
        parts.append(child(parent, "parts"))
        one.append(child(root, "one"))
        print("resident", parts[-1]["wall_ms_per_feed_median"], one[-1]["wall_ms_per_feed_median"], file=sys.stderr, flush=True)
    assert all(r["runs"] == one[0]["runs"] for r in one + parts), [r["runs"] for r in one + parts]
    wall_one, wall_parts = summary(one, "wall_ms_per_feed_median"), summary(parts, "wall_ms_per_feed_median")
    return {"residents": residents, "arriving_videos": videos, "items_per_video": items, "items_held": held, "chunk_items": CHUNK,
            "live_problems": residents * videos + videos * (videos - 1) // 2, "runs": one[0]["runs"],
            "resident_cells_per_feed": CHUNK * videos * residents * (items - 1),
            "launches_in_the_process": {"one_object": one[0]["launches"], "matcher_plus_crossmatcher": parts[0]["launches"]},
            "state_bytes": {"one_object": one[0]["state_bytes"], "matcher_plus_crossmatcher": parts[0]["state_bytes"]},
            "fill_to_level_s": {"one_object": summary(one, "fill_to_level_s"), "matcher_plus_crossmatcher_on_the_parent": summary(parts, "fill_to_level_s")},
            "wall_ms_per_feed": {"one_object": wall_one, "matcher_plus_crossmatcher_on_the_parent": wall_parts},
            "kernel_ms_per_feed_sum": {"one_object": summary(one, "kernel_ms_per_feed_sum"),
                                       "matcher_plus_crossmatcher_on_the_parent": summary(parts, "kernel_ms_per_feed_sum")},
            "kernel_ms_per_feed": {"one_object": one[0]["kernel_ms_per_feed"], "matcher_plus_crossmatcher_on_the_parent": parts[0]["kernel_ms_per_feed"]},
            "condition_one_within_yardstick_plus_its_spread": wall_one["median"] <= wall_parts["median"] + wall_parts["spread"],
            "ratio_parts_to_one": round(wall_parts["median"] / wall_one["median"], 3)}


def bench_resources(root, parent):
    BM.RESOURCE_FILES = ["crossmatch.hip", "matcher.hip", "search.hip", "fingerprint.hip", "fingerprint32.hip", "feeder.hip"]
    this = BM.kernel_resources(root)
    new = {k: v for k, v in sorted(this.items()) if k.startswith("crossmatch_")}
    res = {"how": "hipcc -Rpass-analysis=kernel-resource-usage, gfx950, the Makefile's flags", "crossmatch_kernels": new,
           "crossmatch_kernels_use_no_scratch": all(v.get("scratch", 0) == 0 for v in new.values())}
    if parent:
        before = BM.kernel_resources(parent)
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
    """bench.py on both trees, `repeats` runs each; which tree goes first alternates, so that drift over the runs falls on both."""
    def once(tree):
        run = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree,
                             stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=600, check=True)
        return json.loads(run.stdout.strip().splitlines()[-1])["value"]
    values, order = {"parent": [], "this": []}, []
    for k in range(repeats):
        for name in (("parent", "this") if k % 2 == 0 else ("this", "parent")):
            values[name].append(once(parent if name == "parent" else root))
            order.append(name)
        print("headline", values["parent"][-1], values["this"][-1], file=sys.stderr, flush=True)
    med = {k: statistics.median(v) for k, v in values.items()}
    return {"unit": "bench.py's value", "order": order, "runs": values, "median": med,
            "this_within_parents_spread": min(values["parent"]) <= med["this"] <= max(values["parent"]) or med["this"] >= med["parent"],
            "difference_percent": round(100.0 * (med["this"] - med["parent"]) / med["parent"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="per_feed,tail,season,resources,regions,resident,headline")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, built (yardstick, resources, headline)")
    ap.add_argument("--repeats", type=int, default=4, help="headline runs per tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crossmatch_bench.json"))
    args = ap.parse_args()
    if args.parent:
        args.parent = os.path.abspath(args.parent)
    from needle_amd import capi
    only = set(args.only.split(","))
    keys = ("device", "per_feed", "tail", "season", "resources", "regions", "resident", "headline_vs_parent")
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
    if capi.device_count() > 0:
        res["device"] = capi.device_pci_bus_id()
        for name, run in (("tail", lambda: bench_tail(capi, args.parent)), ("season", lambda: bench_season(capi)),
                          ("per_feed", lambda: bench_per_feed(capi))):
            if name in only:
                res[name] = run()
                save()
        if "regions" in only and args.parent:
            res["regions"] = bench_regions(ROOT, args.parent)
            save()
        if "resident" in only and args.parent:
            res["resident"] = bench_resident(ROOT, args.parent)
            save()
        if "headline" in only and args.parent:
            res["headline_vs_parent"] = bench_headline(ROOT, args.parent, args.repeats)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
