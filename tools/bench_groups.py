"""A library of many shows searched three ways: prints one JSON document.

SHOWS x PER_SHOW videos of 45 minutes (80 x 25 = 2 000 by default; synthetic tonal episodes generated on the device,
synth.DeviceLibrary, one intro of 60 s per show, the default opening window of 50 %, analyzed once and reused):
  grouped    : ONE call, Comparator.run_with_frame_hashes(groups=show of every video) -- sum n_g (n_g - 1) / 2 pairs
  per_show   : the way without groups: a loop of SHOWS ungrouped calls, one per show
  all_pairs  : ONE ungrouped call over everything, n (n - 1) / 2 pairs
Per leg: wall time (median of --steps after --warmup) and, from one more call with the event timers on, the kernel times
(scan = hamming_runs + hamming_runs_unstaged + simhash_runs; epilogue_buckets + epilogue_entries, epilogue_best_match --
per_show stays under the device epilogue's threshold, its epilogue is the host's and inside the wall time only).
differs_grouped_vs_per_show must be 0; differs_grouped_vs_all_pairs counts the videos all pairs answers differently.

Usage: python tools/bench_groups.py [--shows 80] [--per-show 25] [--steps 5] [--warmup 1] [--out profiles/groups_bench.json]"""
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
EPILOGUE = ("epilogue_buckets", "epilogue_entries", "epilogue_best_match")


def analyze(shows, per_show):
    """Every show's opening windows, generated (its own intro) and fingerprinted on the device, show by show."""
    out = []
    for g in range(shows):
        gen = synth.DeviceLibrary(per_show, WINDOW, 60.0, first_episode=g * per_show, intro_seed=synth.INTRO_SEED + 7919 * g)
        lib = capi.Library(per_show, opening_search_percentage=1.0)
        lib.set_pcm_device(gen.pointers(), [WINDOW] * per_show)
        lib.analyze()
        out += [lib.frame_hashes(v) for v in range(per_show)]
        gen.free()
        del lib
    return out


def timed(fn):
    capi.synchronize()
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def plain(results):
    return [None if r is None else (r.opening, r.ending) for r in results]


def measure(fn, steps, warmup):
    walls = []
    for rep in range(warmup + steps):
        ms, out = timed(fn)
        if rep >= warmup:
            walls.append(ms)
    capi.set_kernel_timing(",".join(SCAN + EPILOGUE) + ",sum")   # one more call: every launch of it adds up
    fn()
    kernels = {k: round(v, 4) for k in SCAN + EPILOGUE for v in [capi.last_kernel_ms(k)] if v >= 0}
    launches = {k: capi.kernel_launches(k) for k in SCAN + EPILOGUE if capi.kernel_launches(k)}
    capi.set_kernel_timing(None)
    return {"wall_ms": round(statistics.median(walls), 3), "wall_ms_all": [round(w, 3) for w in walls],
            "scan_kernel_ms": round(sum(v for k, v in kernels.items() if k in SCAN), 4),
            "epilogue_kernel_ms": round(sum(v for k, v in kernels.items() if k in EPILOGUE), 4),
            "kernels_ms": kernels, "launches": launches}, plain(out)


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
    fhs = analyze(shows, per)
    paths = [f"show{v // per:03d}/ep{v % per:02d}.mkv" for v in range(n)]
    labels = [v // per for v in range(n)]
    whole = capi.Comparator(paths)
    each = [capi.Comparator(paths[g * per:(g + 1) * per]) for g in range(shows)]

    def per_show():
        out = []
        for g in range(shows):
            out += each[g].run_with_frame_hashes(fhs[g * per:(g + 1) * per])
        return out

    doc = {"shows": shows, "per_show": per, "videos": n, "minutes": EPISODE_S / 60, "hashes_per_video": len(fhs[0].opening_data()[0]),
           "pairs_grouped": int(len(capi.group_pairs(labels))), "pairs_all": n * (n - 1) // 2, "machine": "AMD Instinct MI355X (gfx950), one GPU",
           "steps": args.steps, "warmup": args.warmup}
    doc["grouped"], grouped = measure(lambda: whole.run_with_frame_hashes(fhs, groups=labels), args.steps, args.warmup)
    doc["per_show"], looped = measure(per_show, args.steps, args.warmup)
    doc["all_pairs"], everything = measure(lambda: whole.run_with_frame_hashes(fhs), args.steps, args.warmup)
    doc["differs_grouped_vs_per_show"] = sum(1 for a, b in zip(grouped, looped) if a != b)
    doc["differs_grouped_vs_all_pairs"] = sum(1 for a, b in zip(grouped, everything) if a != b)
    doc["videos_with_opening_grouped"] = sum(1 for r in grouped if r is not None and r[0] is not None)
    doc["grouped_over_per_show"] = round(doc["grouped"]["wall_ms"] / doc["per_show"]["wall_ms"], 3)
    doc["epilogue_host_fallbacks"] = capi.epilogue_host_fallbacks()
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if doc["differs_grouped_vs_per_show"]:
        sys.exit("grouped and per-show results differ")


if __name__ == "__main__":
    main()
