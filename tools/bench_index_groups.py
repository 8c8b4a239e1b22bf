"""A library of many shows that grows in place: the grouped incremental index against the two ways without it.  Prints one
JSON document.

SHOWS x PER_SHOW videos of 45 minutes (80 x 25 = 2 000 by default; tools/bench_groups.py's library: synthetic tonal episodes
generated on the device, one intro of 60 s per show, the default opening window of 50 %, analyzed once and reused).  A grouped
index (capi.Index(comparator, grouped=True)) holds the library.  Timed, medians of --steps after --warmup, each operation
undone (untimed) before the next repetition:
  append_1 / append_8 : one / eight episodes of one show arrive (they were removed from the index before; they join the end of the list)
  remove_1            : one episode leaves (the list's last)
  replace_1           : one episode is replaced in place
Beside every operation: ONE grouped comparator call over the list the operation leaves (Comparator.run_with_frame_hashes(groups=...),
which searches every pair of every show again), timed in the same process; and, for the appends, the same append to a PLAIN
index of all the videos (n - k resident: it scans k n pairs and ranks every video against all others).  Kernel times come from
one more repetition with the event timers on (scan = hamming_runs + hamming_runs_unstaged + simhash_runs; the index's
index_buckets, index_entries, index_best_match, index_rebuild, index_gather, index_copy_rows).
The tool fails if the grouped index's results ever differ from the grouped call's over the same list.

Usage: python tools/bench_index_groups.py [--shows 80] [--per-show 25] [--steps 5] [--warmup 1] [--out profiles/index_groups_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from needle_amd import capi  # noqa: E402
from tools.bench_groups import analyze, plain  # noqa: E402

SCAN = ("hamming_runs", "hamming_runs_unstaged", "simhash_runs")
INDEX = ("index_buckets", "index_entries", "index_best_match", "index_rebuild", "index_gather", "index_copy_rows")
EPILOGUE = ("epilogue_buckets", "epilogue_entries", "epilogue_best_match")


def timed(fn):
    capi.synchronize()
    t = time.perf_counter()
    fn()
    capi.synchronize()
    return (time.perf_counter() - t) * 1e3


def measure(do, undo, steps, warmup, names):
    """do() timed steps times after warmup, undo() (untimed) after each; then once more with the event timers on."""
    walls = []
    for rep in range(warmup + steps):
        ms = timed(do)
        if rep >= warmup:
            walls.append(ms)
        undo()
    capi.set_kernel_timing(",".join(names) + ",sum")
    do()
    capi.synchronize()
    kernels = {k: round(v, 4) for k in names for v in [capi.last_kernel_ms(k)] if v >= 0}
    capi.set_kernel_timing(None)
    undo()
    return {"wall_ms": round(statistics.median(walls), 3), "wall_ms_all": [round(w, 3) for w in walls],
            "scan_kernel_ms": round(sum(v for k, v in kernels.items() if k in SCAN), 4),
            "other_kernel_ms": round(sum(v for k, v in kernels.items() if k not in SCAN), 4), "kernels_ms": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shows", type=int, default=80)
    ap.add_argument("--per-show", type=int, default=25)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shows, per = args.shows, args.per_show
    n = shows * per
    k8 = min(8, per - 1)
    fhs = analyze(shows, per)
    labels = [v // per for v in range(n)]
    cmp = capi.Comparator([f"show{v // per:03d}/ep{v % per:02d}.mkv" for v in range(n)])
    show = shows // 2                                   # the show that changes: in the middle of the list
    last = [show * per + per - 1 - q for q in range(k8)][::-1]   # its last eight episodes' positions, ascending

    doc = {"shows": shows, "per_show": per, "videos": n, "minutes": 45.0, "hashes_per_video": len(fhs[0].opening_data()[0]),
           "machine": "AMD Instinct MI355X (gfx950), one GPU", "steps": args.steps, "warmup": args.warmup}

    # ---- the grouped index: built show by show, then the episodes that will arrive taken out
    grouped = capi.Index(cmp, grouped=True)
    doc["build_grouped_ms"] = round(timed(lambda: [grouped.add(fhs[g * per:(g + 1) * per], groups=labels[g * per:(g + 1) * per])
                                                   for g in range(shows)]), 3)
    doc["pairs_searched_build"] = grouped.pairs_searched()[0]
    order = list(range(n))                              # the index's current list, as positions of fhs

    def same_as_grouped_call(what):
        want = plain(cmp.run_with_frame_hashes([fhs[p] for p in order], groups=[labels[p] for p in order]))
        if plain(grouped.results()) != want:
            sys.exit(f"{what}: the grouped index's results differ from the grouped call's over the same list")
        return sum(1 for r in want if r is not None and r[0] is not None)

    doc["videos_with_opening"] = same_as_grouped_call("build")

    def leave(index, positions, mirror):
        index.remove(positions)
        for p in sorted(positions, reverse=True):
            del mirror[p]

    def arrive(index, ids, mirror, with_labels):
        if with_labels:
            index.add([fhs[p] for p in ids], groups=[labels[p] for p in ids])
        else:
            index.add([fhs[p] for p in ids])
        mirror += ids

    def call_over(mirror):
        return lambda: cmp.run_with_frame_hashes([fhs[p] for p in mirror], groups=[labels[p] for p in mirror])

    def tail_positions(mirror, k):
        return list(range(len(mirror) - k, len(mirror)))

    for k in (1, k8):
        ids = last[-k:]
        leave(grouped, [order.index(p) for p in ids], order)
        leg = measure(lambda: arrive(grouped, ids, order, True), lambda: leave(grouped, tail_positions(order, k), order), args.steps,
                      args.warmup, SCAN + INDEX)
        arrive(grouped, ids, order, True)
        leg["pairs_scanned"] = grouped.pairs_scanned()[1]
        same_as_grouped_call(f"append_{k}")
        leg["grouped_call"] = measure(call_over(order), lambda: None, args.steps, args.warmup, SCAN + EPILOGUE)
        doc[f"append_{k}"] = leg

    gone = order[-1]                                    # the list's last video (an episode of the show that grew)
    leg = measure(lambda: leave(grouped, [len(order) - 1], order), lambda: arrive(grouped, [gone], order, True), args.steps, args.warmup,
                  SCAN + INDEX)
    leave(grouped, [len(order) - 1], order)
    same_as_grouped_call("remove_1")
    leg["grouped_call"] = measure(call_over(order), lambda: None, args.steps, args.warmup, SCAN + EPILOGUE)
    doc["remove_1"] = leg

    at = order.index(show * per + 5)
    was = order[at]

    def swap(new):
        grouped.replace([at], [fhs[new]])
        order[at] = new

    leg = measure(lambda: swap(gone), lambda: swap(was), args.steps, args.warmup, SCAN + INDEX)   # (the episode just removed: of this show)
    swap(gone)
    leg["pairs_scanned"] = grouped.pairs_scanned()[1]
    same_as_grouped_call("replace_1")
    leg["grouped_call"] = measure(call_over(order), lambda: None, args.steps, args.warmup, SCAN + EPILOGUE)
    doc["replace_1"] = leg
    doc["store_sizes_grouped"] = list(grouped.store_sizes())
    del grouped

    # ---- the same appends to a plain index of all the videos
    ungrouped = capi.Index(cmp)
    flat = [p for p in range(n) if p not in last]
    doc["build_plain_ms"] = round(timed(lambda: ungrouped.add([fhs[p] for p in flat])), 3)
    for k in (1, k8):
        ids = last[-k:]
        leg = measure(lambda: arrive(ungrouped, ids, flat, False), lambda: leave(ungrouped, tail_positions(flat, k), flat), args.steps,
                      args.warmup, SCAN + INDEX)
        arrive(ungrouped, ids, flat, False)
        leg["pairs_scanned"] = ungrouped.pairs_scanned()[1]
        leave(ungrouped, tail_positions(flat, k), flat)
        doc[f"append_{k}"]["plain_index"] = leg
    doc["store_sizes_plain"] = list(ungrouped.store_sizes())
    for k in (1, k8):
        leg = doc[f"append_{k}"]
        leg["over_grouped_call"] = round(leg["wall_ms"] / leg["grouped_call"]["wall_ms"], 3)
        leg["over_plain_index"] = round(leg["wall_ms"] / leg["plain_index"]["wall_ms"], 3)
    for name in ("remove_1", "replace_1"):
        doc[name]["over_grouped_call"] = round(doc[name]["wall_ms"] / doc[name]["grouped_call"]["wall_ms"], 3)
    doc["epilogue_host_fallbacks"] = capi.epilogue_host_fallbacks()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
