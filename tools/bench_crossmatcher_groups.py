#!/usr/bin/env python3
"""Several shows decoded at once: the grouped cross-matcher against the two ways without it -> profiles/crossmatcher_groups_bench.json.

SHOWS x PER_SHOW lanes (16 x 16 = 256 by default) of the tonal 45-minute opening shape (tools/bench_groups.py's library:
synthetic episodes generated on the device, one intro of 60 s per show, analyzed once; 5 441 hashes a lane), fed in equal
chunks of --chunk items per lane, in one process:
  one_grouped_object   : ONE cross-matcher with groups (CrossMatcher.with_groups): the same-label pairs only
  one_object_per_show  : SHOWS ungrouped cross-matchers, fed in turn (3 launches per feed per show)
  one_ungrouped_object : one ungrouped cross-matcher over all lanes (every cross-show pair evaluated and paid state for)
Every object is first filled to --held items per lane (untimed).  Then, --repeats times: 30 feeds timed one by one after 10
untimed (the block's median is the sample), and in a pass of its own 30 feeds under the event timers (the three kernels' mean
per feed).  Reported: the median of the samples, every sample, state bytes (stats[3]) and cells per feed (stats[2]).  At the
end everything is fed and finished, and the tool FAILS if the per-show objects' runs, re-numbered, or the ungrouped object's
runs of same-label pairs, re-numbered, differ from the grouped object's.
  --index        : one season of 8 streamed into the SHOWS_I x PER_I (80 x 25 = 2 000) grouped index
                   (Index.crossmatcher(groups=...) -> add_matched) against Index.add(groups=...) of the same 8: wall ms of
                   the append alone (the feeds overlap the decode and are not part of it), medians of --repeats; the tool fails
                   if the two indexes' results differ.

Usage: python tools/bench_crossmatcher_groups.py [--shows 16] [--per-show 16] [--held 1100] [--chunk 4] [--repeats 5] [--index]
                                                 [--out profiles/crossmatcher_groups_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from needle_amd import capi  # noqa: E402
from tools.bench_groups import analyze, plain  # noqa: E402

KERNELS = ("crossmatch_land", "crossmatch_walk", "crossmatch_simhash")
THRESHOLD, MIN_LEN = 10, 80


class Leg:
    """One alternative: its objects, and which lanes (positions of the lane list) each of them takes."""

    def __init__(self, name, objects, lanes_of):
        self.name, self.objects, self.lanes_of = name, objects, lanes_of
        self.samples, self.kernels = [], []

    def feed(self, data, a, b):
        for o, lanes in zip(self.objects, self.lanes_of):
            o.feed([data[v][a:b] for v in lanes])

    def timed(self, data, pos, count, chunk):
        out = []
        for _ in range(count):
            t0 = time.perf_counter()
            self.feed(data, pos, pos + chunk)
            out.append((time.perf_counter() - t0) * 1e3)
            pos += chunk
        return out, pos

    def stats(self):
        return [sum(o.stats()[k] for o in self.objects) for k in range(4)]


def by_problem(runs):
    out = {}
    for x in runs:
        out.setdefault(int(x["problem"]), []).append(tuple(int(v) for v in x)[1:])
    return {k: sorted(v) for k, v in out.items()}


def crossmatcher_leg(shows, per, held, chunk, repeats):
    n = shows * per
    fhs = analyze(shows, per)
    data = [fh.opening_data()[0] for fh in fhs]
    items = min(len(x) for x in data)
    labels = [v // per for v in range(n)]
    need = held + repeats * 70 * chunk
    assert need <= items, f"{need} items needed, the lanes hold {items}"
    legs = [Leg("one_grouped_object", [capi.CrossMatcher.with_groups(labels, [items], [MIN_LEN], THRESHOLD)], [list(range(n))]),
            Leg("one_object_per_show", [capi.CrossMatcher(per, items, MIN_LEN, THRESHOLD) for _ in range(shows)],
                [list(range(g * per, (g + 1) * per)) for g in range(shows)]),
            Leg("one_ungrouped_object", [capi.CrossMatcher(n, items, MIN_LEN, THRESHOLD)], [list(range(n))])]
    doc = {"shows": shows, "per_show": per, "lanes": n, "items_per_lane": items, "items_held": held, "chunk_items": chunk,
           "repeats": repeats, "live_pairs": {"grouped": shows * per * (per - 1) // 2, "ungrouped_all": n * (n - 1) // 2}}
    pos = {}
    for leg in legs:
        t0 = time.perf_counter()
        leg.feed(data, 0, held)
        capi.synchronize()
        leg.fill_s = time.perf_counter() - t0
        pos[leg.name] = held
    cells = {}
    for _ in range(repeats):                                                     # the three alternate
        for leg in legs:
            _, at = leg.timed(data, pos[leg.name], 10, chunk)
            before = leg.stats()
            wall, at = leg.timed(data, at, 30, chunk)
            after = leg.stats()
            capi.set_kernel_timing(",".join(KERNELS) + ",sum")
            _, at = leg.timed(data, at, 30, chunk)
            capi.synchronize()
            leg.kernels.append({k: capi.last_kernel_ms(k) / 30 for k in KERNELS})
            capi.set_kernel_timing(None)
            leg.samples.append(statistics.median(wall))
            cells[leg.name] = (after[2] - before[2]) // 30
            leg.launches = (after[1] - before[1]) // 30
            pos[leg.name] = at
    for leg in legs:
        doc[leg.name] = {"wall_ms_per_feed": {"median": round(statistics.median(leg.samples), 5), "samples": [round(x, 5) for x in leg.samples]},
                         "kernel_ms_per_feed": {k: round(statistics.median(s[k] for s in leg.kernels), 5) for k in KERNELS},
                         "launches_per_feed": leg.launches, "cells_per_feed_last_block": cells[leg.name], "state_bytes": leg.stats()[3],
                         "fill_to_level_s": round(leg.fill_s, 3)}
        print(leg.name, doc[leg.name], file=sys.stderr, flush=True)
    # the same answer: everything in, finished, compared under the grouped ids
    for leg in legs:
        leg.feed(data, pos[leg.name], items)
        for o in leg.objects:
            o.finish()
    want = by_problem(legs[0].objects[0].runs())
    ids = {tuple(int(x) for x in p): k for k, p in enumerate(capi.group_pairs(labels))}
    local = [(a, b) for a in range(per) for b in range(a + 1, per)]
    per_show = {}
    for g, o in enumerate(legs[1].objects):
        for prob, runs in by_problem(o.runs()).items():
            a, b = local[prob]
            per_show[ids[(g * per + a, g * per + b)]] = runs
    everything = by_problem(legs[2].objects[0].runs())
    every = [(a, b) for a in range(n) for b in range(a + 1, n)]
    same_label = {ids[every[prob]]: runs for prob, runs in everything.items() if labels[every[prob][0]] == labels[every[prob][1]]}
    if per_show != want or same_label != want:
        sys.exit("the alternatives' runs differ from the grouped cross-matcher's")
    doc["problems_with_runs"] = {"grouped": len(want), "ungrouped_all": len(everything)}
    doc["runs"] = {"grouped": sum(len(v) for v in want.values()), "ungrouped_all": sum(len(v) for v in everything.values())}
    doc["derived_state_bytes"] = {"grouped": capi.CrossMatcher.state_bytes_grouped(labels, [items]),
                                  "ungrouped_all": capi.CrossMatcher.state_bytes(n, items)}
    return doc


def index_leg(shows, per, repeats, k=8):
    n = shows * per
    fhs = analyze(shows, per)
    labels = [v // per for v in range(n)]
    cmp = capi.Comparator([f"show{v // per:03d}/ep{v % per:02d}.mkv" for v in range(n)])
    show = shows // 2
    ids = [show * per + per - k + q for q in range(k)]                           # the show's last eight episodes arrive
    rest = [v for v in range(n) if v not in ids]
    streamed, added = capi.Index(cmp, grouped=True), capi.Index(cmp, grouped=True)
    for ix in (streamed, added):
        for g in range(shows):
            members = [v for v in rest if labels[v] == g]
            ix.add([fhs[v] for v in members], groups=[g] * len(members))
    new, rows = [fhs[v] for v in ids], [fhs[v].opening_data()[0] for v in ids]
    walls = {"add_matched": [], "add_grouped": [], "crossmatcher_feed_and_finish": []}
    for _ in range(repeats + 1):                                                 # (the first is the warm-up)
        m = streamed.crossmatcher(k, [max(len(x) for x in rows)], [20], groups=[show] * k)   # (a lower bound: the ingest applies each pair's own)
        capi.synchronize()
        t0 = time.perf_counter()
        m.feed(rows)
        m.finish()
        walls["crossmatcher_feed_and_finish"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        streamed.add_matched(m, new)
        capi.synchronize()
        walls["add_matched"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        added.add(new, groups=[show] * k)
        capi.synchronize()
        walls["add_grouped"].append((time.perf_counter() - t0) * 1e3)
        if plain(streamed.results()) != plain(added.results()) or streamed.store_sizes() != added.store_sizes():
            sys.exit("the streamed append's results differ from add_grouped's")
        for ix in (streamed, added):
            ix.remove(list(range(n - k, n)))
    return {"shows": shows, "per_show": per, "videos": n, "arriving": k, "live_pairs": k * (per - k) + k * (k - 1) // 2,
            "wall_ms": {name: {"median": round(statistics.median(v[1:]), 3), "samples": [round(x, 3) for x in v[1:]]} for name, v in walls.items()},
            "pairs_scanned_last": {"add_matched": 0, "add_grouped": k * (per - k) + k * (k - 1) // 2}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shows", type=int, default=16)
    ap.add_argument("--per-show", type=int, default=16)
    ap.add_argument("--held", type=int, default=1100)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--index", action="store_true")
    ap.add_argument("--index-shows", type=int, default=80)
    ap.add_argument("--index-per-show", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crossmatcher_groups_bench.json"))
    args = ap.parse_args()
    if capi.device_count() < 1:
        sys.exit("needs a HIP device")
    doc = {"machine": "AMD Instinct MI355X (gfx950), one GPU", "device": capi.device_pci_bus_id(),
           "crossmatcher": crossmatcher_leg(args.shows, args.per_show, args.held, args.chunk, args.repeats), "index": "not measured"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    if args.index:
        doc["index"] = index_leg(args.index_shows, args.index_per_show, args.repeats)
        json.dump(doc, open(args.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
