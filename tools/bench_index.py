"""Cost of growing a library with the incremental index (needle_hip_index_*): prints one JSON document.

For N = 250, 500 and 1000 videos of 45 minutes (synthetic tonal episodes generated on the device, synth.DeviceLibrary, the
default opening window of 50 %, analyzed once and reused):
  append_1 / append_8   : wall time of needle_hip_index_add of 1 / 8 new videos to an index holding N
  full_1 / full_8       : wall time of needle_hip_comparator_run_with_frame_hashes over the same N + 1 / N + 8 videos
  kernels               : event-timed kernel milliseconds of one such call (scan = hamming_runs + simhash_runs; the index's
                          entries = index_buckets + index_entries, its best match = index_best_match; the full search's
                          epilogue_buckets + epilogue_entries and epilogue_best_match), from a separate pass with timing on
Medians over --steps calls after --warmup.

--matched: a streamed season into the index (needle_hip_index_crossmatcher_new, needle_hip_index_add_matched) with
--resident K known videos and --arriving N new ones (1 000 and 28), one region, in place of the sizes above:
  add_matched           : wall time of needle_hip_index_add_matched from a complete matcher, and its kernels (index_ingest in
                          place of the scan's)
  add                   : the same for needle_hip_index_add of the same N videos on the same index state
  crossmatcher_from_index / crossmatcher_from_host : wall time of needle_hip_index_crossmatcher_new (rows gathered from the
                          store's arena: crossmatch_gather_resident) against needle_hip_crossmatcher_new_resident over a
                          host arena that is already packed
  feed_s                : what the search cost while the season "decoded": every lane fed in strips of 512 hashes

Usage: python tools/bench_index.py [--sizes 250,500,1000] [--steps K] [--warmup W] [--out profiles/index_bench.json]
       python tools/bench_index.py --matched [--resident K] [--arriving N] [--steps K] [--warmup W] [--out ...]

--streamed: the same shape through both routes side by side -- one cross-matcher with residents and add_matched, against the
matcher made from the index, the arriving pairs' cross-matcher and add_streamed (needle_hip_index_matcher_new,
needle_hip_index_add_streamed): creation, feed time, the final add and the state bytes of each.
       python tools/bench_index.py --streamed [--resident K] [--arriving N] [--steps K] [--warmup W] [--out ...]

--evidence: the cost of needle_hip_index_evidence over an index holding N videos of the sizes above: wall time of the call
(into a buffer made before) and the event times of its two kernels (index_evidence_match = best_match_kernel over every video
with the winners written out, index_evidence = match_evidence_kernel), medians of 5 calls after one warm-up; beside them
index_best_match of the append of the N-th video onto N - 1, the figure an append pays for the videos it changed.
       python tools/bench_index.py --evidence [--sizes 250,500,1000] [--out profiles/index_evidence_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

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


MATCHED = ("index_ingest",) + INDEX
GATHER = ("crossmatch_gather_resident",)


def fed_matcher(index, rows, cap, min_len):
    """A complete matcher made from `index` over the lanes `rows`, fed in strips; (matcher, creation ms, feed seconds)."""
    made = []
    ms = timed(lambda: made.append(index.crossmatcher(len(rows), cap, min_len)))
    m = made[0]
    t = time.perf_counter()
    for at in range(0, max(len(x) for x in rows), 512):
        m.feed([x[at:at + 512] for x in rows])
    m.finish()
    assert m.ready()[1]
    return m, ms, time.perf_counter() - t


def bench_matched(fhs, n, k, steps, warmup):
    new = fhs[n:n + k]
    rows = [fh.opening_data()[0] for fh in new]
    cap = [max(len(x) for x in rows)]
    ts = new[0].opening_data()[1]
    min_len = [int(-(-capi.DEFAULT_MIN_OPENING_DURATION * 10 ** 9 // int(ts[1] - ts[0])))]   # evenly spaced timestamps: the index's own bound
    resident = [fh.opening_data()[0] for fh in fhs[:n]]
    arena = np.concatenate(resident)
    seqs = np.zeros((n, 2), dtype=np.uint32)
    seqs[:, 1] = [len(x) for x in resident]
    seqs[:, 0] = np.cumsum([0] + [len(x) for x in resident])[:n]
    matched, plain, from_index, from_host, feeds, runs = [], [], [], [], [], 0
    want = None
    for rep in range(warmup + steps + 1):
        timing = rep == warmup + steps          # one more pass with the event timers on
        a, b = capi.Index(comparator(n)), capi.Index(comparator(n))
        a.add(fhs[:n])
        b.add(fhs[:n])
        if timing:
            capi.set_kernel_timing(",".join(GATHER) + ",sum")
        m, made_ms, feed_s = fed_matcher(a, rows, cap, min_len)
        if timing:
            gather_k = kernel_ms(GATHER)
        h = C.c_void_p()
        host_ms = timed(lambda: capi.check(capi.lib().needle_hip_crossmatcher_new_resident(
            arena.ctypes.data, arena.size, seqs.ctypes.data, n, k, 1, (C.c_size_t * 1)(*cap), (C.c_uint32 * 1)(*min_len),
            capi.DEFAULT_HASH_MATCH_THRESHOLD, C.byref(h))))
        capi.lib().needle_hip_crossmatcher_free(h)
        runs = m.ready()[0]
        if timing:
            capi.set_kernel_timing(",".join(SCAN + MATCHED) + ",sum")
        a_ms = timed(lambda: a.add_matched(m, new))
        if timing:
            matched_k = kernel_ms(SCAN + MATCHED)
            capi.set_kernel_timing(",".join(SCAN + INDEX) + ",sum")   # a new selection: the sums start again
        b_ms = timed(lambda: b.add(new))
        if timing:
            plain_k = kernel_ms(SCAN + INDEX)
            capi.set_kernel_timing(None)
        got = [None if r is None else (r.opening, r.ending) for r in a.results()]
        assert got == [None if r is None else (r.opening, r.ending) for r in b.results()], "add_matched and add disagree"
        assert a.store_sizes() == b.store_sizes() and a.pairs_searched() == b.pairs_searched() and a.pairs_scanned()[1] == 0
        if warmup <= rep < warmup + steps:
            matched.append(a_ms)
            plain.append(b_ms)
            from_index.append(made_ms)
            from_host.append(host_ms)
            feeds.append(feed_s)
        del m, a, b
    med = statistics.median
    return {"resident": n, "arriving": k, "matcher_runs": runs, "matcher_min_len": min_len[0],
            "add_matched_ms": round(med(matched), 3), "add_ms": round(med(plain), 3),
            "add_matched_ms_min_max": [round(min(matched), 3), round(max(matched), 3)], "add_ms_min_max": [round(min(plain), 3), round(max(plain), 3)],
            "add_matched_kernels_ms": matched_k, "add_kernels_ms": plain_k,
            "crossmatcher_from_index_ms": round(med(from_index), 3), "crossmatcher_from_host_ms": round(med(from_host), 3),
            "crossmatcher_from_index_kernels_ms": gather_k, "feed_s": round(med(feeds), 3)}


def bench_streamed(fhs, n, k, steps, warmup):
    """The two routes of a streamed season at one shape, side by side: one cross-matcher with residents (add_matched) and
    the matcher made from the index with the arriving pairs' cross-matcher (add_streamed)."""
    new = fhs[n:n + k]
    rows = [fh.opening_data()[0] for fh in new]
    cap = [max(len(x) for x in rows)]
    ts = new[0].opening_data()[1]
    min_len = [int(-(-capi.DEFAULT_MIN_OPENING_DURATION * 10 ** 9 // int(ts[1] - ts[0])))]
    out = {"matched": {"made_ms": [], "feed_s": [], "add_ms": []}, "streamed": {"made_ms": [], "feed_s": [], "add_ms": []}}
    for rep in range(warmup + steps + 1):
        timing = rep == warmup + steps          # one more pass with the event timers on
        a, b = capi.Index(comparator(n)), capi.Index(comparator(n))
        a.add(fhs[:n])
        b.add(fhs[:n])
        m, made_ms, feed_s = fed_matcher(a, rows, cap, min_len)
        made = []
        made2_ms = timed(lambda: made.extend([b.matcher(k), capi.CrossMatcher.with_regions(k, cap, min_len, capi.DEFAULT_HASH_MATCH_THRESHOLD)]))
        mt, cm = made
        t = time.perf_counter()
        for at in range(0, cap[0], 512):
            chunk = [x[at:at + 512] for x in rows]
            mt.feed(chunk)
            cm.feed(chunk)
        mt.finish()
        cm.finish()
        feed2_s = time.perf_counter() - t
        state = {"matched": m.stats()[3], "streamed": mt.stats()[3] + cm.stats()[3]}
        runs = {"matched": m.ready()[0], "streamed": sum(mt.ready(i)[0] for i in range(k)) + cm.ready()[0]}
        if timing:
            capi.set_kernel_timing(",".join(SCAN + MATCHED) + ",sum")
        a_ms = timed(lambda: a.add_matched(m, new))
        if timing:
            out["matched"]["add_kernels_ms"] = kernel_ms(SCAN + MATCHED)
            capi.set_kernel_timing(",".join(SCAN + MATCHED) + ",sum")
        b_ms = timed(lambda: b.add_streamed(mt, cm, new))
        if timing:
            out["streamed"]["add_kernels_ms"] = kernel_ms(SCAN + MATCHED)
            capi.set_kernel_timing(None)
        got = [None if r is None else (r.opening, r.ending) for r in a.results()]
        assert got == [None if r is None else (r.opening, r.ending) for r in b.results()], "add_matched and add_streamed disagree"
        assert a.store_sizes() == b.store_sizes() and a.pairs_searched() == b.pairs_searched() and b.pairs_scanned()[1] == 0
        if warmup <= rep < warmup + steps:
            for route, row in (("matched", (made_ms, feed_s, a_ms)), ("streamed", (made2_ms, feed2_s, b_ms))):
                for key, v in zip(("made_ms", "feed_s", "add_ms"), row):
                    out[route][key].append(v)
        del m, mt, cm, a, b
    for route in ("matched", "streamed"):
        for key in ("made_ms", "feed_s", "add_ms"):
            out[route][key] = round(statistics.median(out[route][key]), 3)
        out[route]["state_bytes"] = state[route]
        out[route]["runs"] = runs[route]
    out.update({"resident": n, "arriving": k, "regions": 1, "min_len": min_len[0], "items_per_video": cap[0],
                "what": "matched: index.crossmatcher + add_matched; streamed: index.matcher + CrossMatcher.with_regions + add_streamed; "
                        "feeds in strips of 512 items, every lane in every feed; medians"})
    return out


EVIDENCE = ("index_evidence_match", "index_evidence")


def bench_evidence(fhs, n, calls=5):
    index = capi.Index(comparator(n))
    index.add(fhs[:n - 1])
    capi.set_kernel_timing("index_best_match,sum")
    index.add(fhs[n - 1:n])
    append = kernel_ms(("index_best_match",))
    capi.set_kernel_timing(None)
    listed = sum(1 for r in index.results() if r is not None)
    ev = (capi.CSearchEvidence * n)()
    call = lambda: capi.check(capi.lib().needle_hip_index_evidence(index._h, ev, n))
    call()                                                       # warm-up: the buffers of its own, the code objects
    wall, kernels = [], {k: [] for k in EVIDENCE}
    for _ in range(calls):
        wall.append(timed(call))
    for _ in range(calls):
        capi.set_kernel_timing(",".join(EVIDENCE) + ",sum")     # a new selection: the sums start again
        call()
        for k, v in kernel_ms(EVIDENCE).items():
            kernels[k].append(v)
        capi.set_kernel_timing(None)
    got = capi._evidence(ev, n)
    results = index.results()
    assert all((e.opening is None) == (r is None or r.opening is None) for e, r in zip(got, results)), "evidence and results disagree"
    med = statistics.median
    return {"videos": n, "videos_with_a_result": listed, "candidates_max": max((e.opening.candidates for e in got if e.opening), default=0),
            "evidence_wall_ms": round(med(wall), 4), "evidence_wall_ms_min_max": [round(min(wall), 4), round(max(wall), 4)],
            "evidence_kernels_ms": {k: round(med(v), 4) for k, v in kernels.items()},
            "append_1_index_best_match_ms": append.get("index_best_match"), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="250,500,1000")
    ap.add_argument("--matched", action="store_true")
    ap.add_argument("--streamed", action="store_true")
    ap.add_argument("--evidence", action="store_true")
    ap.add_argument("--resident", type=int, default=1000)
    ap.add_argument("--arriving", type=int, default=28)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bench_index.py needs a HIP device")
    sizes = [int(x) for x in a.sizes.split(",")] if not (a.matched or a.streamed) else []
    t = time.perf_counter()
    fhs = analyze(a.resident + a.arriving if a.matched or a.streamed else max(sizes) + 8)
    doc = {"machine": "AMD Instinct MI355X (gfx950), one GPU", "device": capi.device_pci_bus_id(), "episode_s": EPISODE_S, "window_hashes": len(fhs[0].opening_data()[0]),
           "analyze_s": round(time.perf_counter() - t, 1), "steps": a.steps, "warmup": a.warmup, "sizes": {}}
    if a.matched:
        del doc["sizes"]
        doc["matched"] = bench_matched(fhs, a.resident, a.arriving, a.steps, a.warmup)
    if a.streamed:
        doc.pop("sizes", None)
        doc["two_routes"] = bench_streamed(fhs, a.resident, a.arriving, a.steps, a.warmup)
    if a.evidence:
        del doc["sizes"]
        doc["evidence"] = {str(n): bench_evidence(fhs, n) for n in sizes}
        sizes = []
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
