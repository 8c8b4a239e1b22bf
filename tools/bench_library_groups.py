"""A library of many shows as library jobs (analyze + search, PCM resident in HBM), three ways: prints one JSON document.

SHOWS x PER_SHOW episodes of 45 minutes (80 x 25 = 2 000 by default; synthetic tonal episodes generated on the device,
synth.DeviceLibrary, one intro of 60 s per show, the opening window of 50 %), one GPU:
  grouped   : ONE NeedleHipLibrary with a label per video (needle_hip_library_set_groups): sum n_g (n_g - 1) / 2 pairs
  plain     : the same PCM as ONE library without labels, all n (n - 1) / 2 pairs -- the only one-object form without groups
  per_show  : SHOWS plain libraries of PER_SHOW, their jobs run one after another
Per form: the median wall time of a steady-state job (a job = job_begin + job_end of every object of the form, the device
drained at its end; --steps timed after --warmup), the same with two jobs in flight (per_show: the next show's job is
enqueued before the last one's is collected), the job's form (needle_hip_library_job_form) and, from one more job with
the event timers on, the kernel times: scan = hamming_runs + hamming_runs_unstaged + simhash_runs, the first pass and the
epilogue's kernels beside it.  grouped and per_show must give the same results; plain answers differently wherever a video
of another show matches better.

Usage: python tools/bench_library_groups.py [--shows 80] [--per-show 25] [--minutes 45] [--steps 5] [--warmup 2]
                                            [--out profiles/library_groups_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from needle_amd import capi, synth  # noqa: E402

SCAN = ("hamming_runs", "hamming_runs_unstaged", "simhash_runs")
ANALYZE = ("stft_chroma32", "features_cert", "stft_fallback", "fixup_items", "stft_chroma", "features_classify")
EPILOGUE = ("epilogue_buckets", "epilogue_entries", "epilogue_best_match")


def plain(results):
    return [None if r is None else (r.opening, r.ending) for r in results]


class Form:
    """A list of (library, comparator) whose jobs, one after another, are one job of the form."""

    def __init__(self, objects):
        self.objects = objects

    def one_at_a_time(self):
        out = []
        for lib, cmp in self.objects:
            lib.job_begin(cmp, 0)
            out += lib.job_end(cmp, 0)[0]
        capi.synchronize()
        return out

    def in_flight(self, jobs):
        """`jobs` jobs of the form with two library jobs in flight throughout (one object: its two slots in turn; several:
        the next object's job is enqueued before the last one's is collected)."""
        pending = []
        seq = 0
        for _ in range(jobs):
            for lib, cmp in self.objects:
                slot = seq & 1 if len(self.objects) == 1 else 0
                seq += 1
                lib.job_begin(cmp, slot)
                if pending:
                    plib, pcmp, pslot = pending.pop()
                    plib.job_end(pcmp, pslot)
                pending.append((lib, cmp, slot))
        while pending:
            plib, pcmp, pslot = pending.pop()
            plib.job_end(pcmp, pslot)
        capi.synchronize()

    def measure(self, steps, warmup):
        for _ in range(warmup):
            self.one_at_a_time()
        walls = []
        for _ in range(steps):
            capi.synchronize()
            t = time.perf_counter()
            res = self.one_at_a_time()
            walls.append(1e3 * (time.perf_counter() - t))
        flights = []
        self.in_flight(2)
        for _ in range(3):
            capi.synchronize()
            t = time.perf_counter()
            self.in_flight(steps)
            flights.append(1e3 * (time.perf_counter() - t) / steps)
        names = SCAN + ANALYZE + EPILOGUE
        capi.set_kernel_timing(",".join(names) + ",sum")         # one more job: every launch of it adds up
        self.one_at_a_time()
        kernels = {k: round(v, 4) for k in names for v in [capi.last_kernel_ms(k)] if v > 0}
        launches = {k: capi.kernel_launches(k) for k in names if capi.kernel_launches(k)}
        capi.set_kernel_timing(None)
        lib = self.objects[0][0]
        return {"wall_ms": round(statistics.median(walls), 3), "wall_ms_all": [round(w, 3) for w in walls],
                "wall_ms_two_in_flight": round(statistics.median(flights), 3), "wall_ms_two_in_flight_all": [round(w, 3) for w in flights],
                "job_form": lib.job_form(0), "pairs": sum(l.num_pairs() for l, _ in self.objects),
                "scan_kernel_ms": round(sum(v for k, v in kernels.items() if k in SCAN), 4),
                "analyze_kernel_ms": round(sum(v for k, v in kernels.items() if k in ANALYZE), 4),
                "epilogue_kernel_ms": round(sum(v for k, v in kernels.items() if k in EPILOGUE), 4),
                "kernels_ms": kernels, "launches": launches}, plain(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shows", type=int, default=80)
    ap.add_argument("--per-show", type=int, default=25)
    ap.add_argument("--minutes", type=float, default=45.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if capi.device_count() < 1:
        sys.exit("bench_library_groups.py needs a HIP device: the library job has no CPU fallback")
    shows, per = args.shows, args.per_show
    n = shows * per
    window = int(args.minutes * 60 * capi.DEFAULT_OPENING_SEARCH_PERCENTAGE * synth.RATE)
    # every show's opening windows, generated in HBM with the show's own intro; kept until the last form has copied them
    gens = [synth.DeviceLibrary(per, window, 60.0, first_episode=g * per, intro_seed=synth.INTRO_SEED + 7919 * g) for g in range(shows)]
    pointers = [p for gen in gens for p in gen.pointers()]
    paths = [f"show{v // per:03d}/ep{v % per:02d}.mkv" for v in range(n)]
    labels = [v // per for v in range(n)]

    def library(first, count, groups=None):
        lib = capi.Library(count, opening_search_percentage=1.0)
        if groups is not None:
            lib.set_groups(groups)
        lib.set_pcm_device(pointers[first:first + count], [window] * count)
        return lib, capi.Comparator(paths[first:first + count])

    doc = {"shows": shows, "per_show_videos": per, "videos": n, "minutes": args.minutes,
           "hashes_per_video": int(capi.lib().needle_hip_fingerprint_num_kept(window, 2)),
           "pairs_grouped": int(len(capi.group_pairs(labels))), "pairs_all": n * (n - 1) // 2,
           "machine": "AMD Instinct MI355X (gfx950), one GPU", "steps": args.steps, "warmup": args.warmup}
    results = {}
    for name, make in (("grouped", lambda: [library(0, n, labels)]), ("plain", lambda: [library(0, n)]),
                       ("per_show", lambda: [library(g * per, per) for g in range(shows)])):
        form = Form(make())                                       # one form's PCM resident at a time
        doc[name], results[name] = form.measure(args.steps, args.warmup)
        del form
    for gen in gens:
        gen.free()
    doc["differs_grouped_vs_per_show"] = sum(1 for a, b in zip(results["grouped"], results["per_show"]) if a != b)
    doc["differs_grouped_vs_plain"] = sum(1 for a, b in zip(results["grouped"], results["plain"]) if a != b)
    doc["videos_with_opening_grouped"] = sum(1 for r in results["grouped"] if r is not None and r[0] is not None)
    doc["grouped_over_plain"] = round(doc["grouped"]["wall_ms"] / doc["plain"]["wall_ms"], 4)
    doc["grouped_over_per_show"] = round(doc["grouped"]["wall_ms"] / doc["per_show"]["wall_ms"], 4)
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
