"""Cost of removing and replacing videos in the incremental index (needle_hip_index_remove / _replace): prints one JSON
document.

For N = 250, 500 and 1000 videos of 45 minutes (the tonal episodes and the analysis step of tools/bench_index.py), on an
index holding N videos whose second set of buffers is already allocated (one edit before the measurements):
  remove_1_first / remove_1_middle : wall time of removing the video at position 0 / N // 2
  remove_8                         : wall time of removing 8 videos spread over the list
  replace_1                        : wall time of replacing the video at N // 2 with one not in the index
  full_*                           : in the same process, wall time of needle_hip_comparator_run_with_frame_hashes over the
                                     list that operation leaves
  *_kernels_ms                     : event-timed kernel milliseconds of one such call, from a separate pass with timing on
  gather                           : the gather kernel's bytes (every entry held read and written once, 48 B each) over its
                                     time, against the 6.29 TB/s a device-to-device copy reaches on one MI355X
After each measured call the index is put back (the removed videos appended again / the replaced one restored); those
calls are not timed.  Medians over --steps calls after --warmup.

Usage: python tools/bench_index_edit.py [--sizes 250,500,1000] [--steps K] [--warmup W] [--out profiles/index_edit_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from needle_amd import capi  # noqa: E402
from bench_index import EPISODE_S, SCAN, analyze, comparator, kernel_ms, timed  # noqa: E402

EDIT = ("index_copy_rows", "index_buckets", "index_entries", "index_rebuild", "index_gather", "index_best_match")
FULL = ("epilogue_buckets", "epilogue_entries", "epilogue_best_match")
COPY_TBPS = 6.29
ENTRY_BYTES = 48


def _as(rs):
    return [None if r is None else (r.opening, r.ending) for r in rs]


class Bench:
    def __init__(self, fhs, n):
        self.fhs, self.n = fhs, n
        self.index = capi.Index(comparator(n))
        self.cur = list(range(n))           # fhs ids, in the index's order
        self.index.add([fhs[v] for v in self.cur])

    def remove(self, positions, restore):
        """Times the removal, then (restore) appends the removed videos again, untimed."""
        gone = [self.cur[p] for p in positions]
        ms = timed(lambda: self.index.remove(positions))
        after = [v for q, v in enumerate(self.cur) if q not in set(positions)]
        self.cur = after + gone if restore else after
        if restore:
            self.index.add([self.fhs[v] for v in gone])
        return ms, after

    def replace(self, position, spare, restore):
        """Times the replacement, then (restore) puts the original back, untimed."""
        was = self.cur[position]
        ms = timed(lambda: self.index.replace([position], [self.fhs[spare]]))
        after = list(self.cur)
        after[position] = spare
        if restore:
            self.index.replace([position], [self.fhs[was]])
        else:
            self.cur = after
        return ms, after

    def op(self, name, restore=True):
        n = self.n
        if name == "remove_1_first":
            return self.remove([0], restore)
        if name == "remove_1_middle":
            return self.remove([n // 2], restore)
        if name == "remove_8":
            return self.remove([k * n // 8 + 3 for k in range(8)], restore)
        return self.replace(n // 2, n, restore)


def bench(fhs, n, steps, warmup):
    out = {}
    b = Bench(fhs, n)
    b.op("remove_1_middle")                 # allocates the second set of buffers
    for name in ("remove_1_first", "remove_1_middle", "remove_8", "replace_1"):
        times, full = [], []
        after = None
        for rep in range(warmup + steps):
            ms, after = b.op(name)
            if rep >= warmup:
                times.append(ms)
        cmp = comparator(len(after))
        for rep in range(warmup + steps):
            t = timed(lambda: cmp.run_with_frame_hashes([fhs[v] for v in after]))
            if rep >= warmup:
                full.append(t)
        # kernel times of one such call with the event timers on ("sum": every launch of the call adds up)
        capi.set_kernel_timing(",".join(SCAN + EDIT) + ",sum")
        _, after = b.op(name, restore=False)
        edit_k = kernel_ms(SCAN + EDIT)
        capi.set_kernel_timing(None)
        got = _as(b.index.results())
        held = b.index.store_sizes()[0]
        assert got == _as(cmp.run_with_frame_hashes([fhs[v] for v in after])), f"{name}: index and full search disagree"
        capi.set_kernel_timing(",".join(SCAN + FULL) + ",sum")
        cmp.run_with_frame_hashes([fhs[v] for v in after])
        full_k = kernel_ms(SCAN + FULL)
        capi.set_kernel_timing(None)
        # put the index back to N videos in the order the Bench expects
        b = Bench(fhs, n)
        b.op("remove_1_middle")
        out[f"{name}_ms"] = round(statistics.median(times), 3)
        out[f"full_{name}_ms"] = round(statistics.median(full), 3)
        out[f"speedup_{name}"] = round(statistics.median(full) / statistics.median(times), 2)
        out[f"{name}_kernels_ms"] = edit_k
        out[f"full_{name}_kernels_ms"] = full_k
        gather_ms = edit_k.get("index_gather", -1)
        if gather_ms > 0:
            moved = 2 * held * ENTRY_BYTES
            out[f"{name}_gather"] = {"entries": held, "bytes": moved, "ms": gather_ms,
                                     "tb_per_s": round(moved / (gather_ms * 1e-3) / 1e12, 3),
                                     "of_copy_rate": round(moved / (gather_ms * 1e-3) / 1e12 / COPY_TBPS, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="250,500,1000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_index_edit.py needs a HIP device")
    sizes = [int(x) for x in a.sizes.split(",")]
    t = time.perf_counter()
    fhs = analyze(max(sizes) + 1)
    doc = {"machine": "AMD Instinct MI355X (gfx950), one GPU", "device": capi.device_pci_bus_id(), "episode_s": EPISODE_S,
           "window_hashes": len(fhs[0].opening_data()[0]), "analyze_s": round(time.perf_counter() - t, 1), "steps": a.steps,
           "warmup": a.warmup, "copy_tb_per_s": COPY_TBPS, "sizes": {}}
    for n in sizes:
        row = bench(fhs, n, a.steps, a.warmup)
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
