"""Cost of feeding PCM in chunks (needle_hip_feeder_*): writes profiles/feeder_bench.json and prints it as one JSON line.

  chunked : the 28 opening windows (12 min) of 28 x 24-min episodes, from pinned host memory, fed in lock-step in chunks of
            0.5 s, 5 s and 60 s and finished, against the one-shot call over the same windows in the same process,
            alternating, median of --repeats (wall time, items on the host at the end of both): s16 mono at 11025 Hz
            against needle_hip_fingerprint_host, 48 kHz planar-float stereo against needle_hip_analyzer_run_pcm_format.
  per_feed: ms per feed at 1, 28 and 256 lanes of 1-s chunks (s16 mono 11025 Hz), median over a minute of audio.
  state   : needle_hip_feeder_state_bytes per lane, by shape.
  launches: kernel launches per feed, by kernel: a child of this tool feeds --trace-feeds seconds into 1, 28 and 256
            lanes under `rocprofv3 --kernel-trace --stats`, a run of its own, and the calls of its statistics are divided
            by the feeds (the carry has nothing to move in a stream's first feed).
  resources: registers, LDS and scratch of the feeder's kernel and of the kernels the feeder shares with the one-shot
            paths, from the compiler's remarks (-Rpass-analysis=kernel-resource-usage, needs no device), for this tree
            and, with --parent DIR (a checkout of the parent commit), for that one; "unchanged" compares the kernels
            both have.
  audit   : the audit that travels with the stream (needle_hip_feeder_set_audit): 28 lanes of 48 kHz planar-float stereo in
            1-s chunks, wall ms per feed with the audit off and on, alternating, median of 30 after 10; the event times
            per feed of the first pass and of the audit's two kernels, from a pass of their own; and, with --parent DIR
            (built), the audit-off leg in five processes of each tree, alternating, the tree that goes first alternating
            too: this tree's median must stay within the parent's median + the spread of the parent's five.
  headline: with --parent DIR (built), bench.py --gpus 1 --steps 20 --warmup 5 in both trees, alternating, --repeats
            times each: medians, the difference and each side's spread (max - min).
  mixed:    28 lanes in four formats through one with_formats feeder against four uniform feeders of seven lanes fed in
            turn: wall ms per feed, the front end's kernel times and launches (not in the default --only).
  uniform:  with --parent DIR, the audit section's comparison with the parent alone: the uniform 28-lane leg, five
            processes per tree (not in the default --only).
  switch:   a lane that changes format in mid-stream (needle_hip_feeder_switch_format; not in the default --only).
            (a) with --parent DIR (built): the uniform leg above and a mixed leg (the 28 lanes of `mixed` through one
            with_formats feeder), neither of which ever switches, five processes per tree, alternating: this tree's median
            must stay within the parent's median + the spread of the parent's five.  (b) one switch call on 28 lanes of
            48 kHz s16 stereo, 7 of them to 44.1 kHz, after 1, 2, ... 10 s of 1-s feeds: wall ms (to the items on the host)
            and summed kernel-event ms of the call, beside the per-feed wall ms of the same feeder; recorded, no target.
Sections not asked for with --only keep the figures the output file already holds.

Usage: python tools/bench_feeder.py [--repeats K] [--episodes N] [--out FILE] [--parent DIR]
                                    [--only chunked,per_feed,state,launches,resources,headline,audit,mixed,uniform,switch]"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from needle_amd import capi, synth  # noqa: E402

NOT_MEASURED = "not measured"


def median_ms(fn, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def feed_all(lanes, ch, rate, fmt, chunk_frames, planar):
    f = capi.Feeder(len(lanes), ch, rate, fmt, 2)
    frames = [(len(x[0]) if planar else len(x) // ch) for x in lanes]
    for pos in range(0, max(frames), chunk_frames):
        if planar:
            f.feed([[p[pos: pos + chunk_frames] for p in x] if pos < n else None for x, n in zip(lanes, frames)])
        else:
            f.feed([x[pos * ch: (pos + chunk_frames) * ch] if pos < n else None for x, n in zip(lanes, frames)])
    f.finish()
    return [f.items(k) for k in range(len(lanes))], f.state_bytes()


def bench_chunked(episodes, repeats):
    eps = synth.make_library(episodes, 24 * 60.0, 90.0)
    out = {}
    # s16 mono at 11025 Hz, pinned
    pinned = []
    for e in eps:
        b = capi.PinnedArray(len(e.pcm) // 2)
        b.array[:] = e.pcm[: len(e.pcm) // 2]
        pinned.append(b)
    wins = [b.array for b in pinned]
    want = capi.fingerprint(wins, 1, 2)
    shape = {"chunks": {}}
    for name, secs in [("0.5s", 0.5), ("5s", 5.0), ("60s", 60.0)]:
        chunk = int(secs * 11025)
        got, _ = feed_all(wins, 1, 11025, capi.SAMPLE_S16, chunk, False)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        one, fed = [], []
        for _ in range(repeats):
            one.append(median_ms(lambda: capi.fingerprint(wins, 1, 2), 1))
            fed.append(median_ms(lambda: feed_all(wins, 1, 11025, capi.SAMPLE_S16, chunk, False), 1))
        shape["chunks"][name] = {"fed_ms": statistics.median(fed), "one_shot_ms": statistics.median(one),
                                 "feeds": -(-len(wins[0]) // chunk)}
        print("s16 mono 11025", name, shape["chunks"][name], file=sys.stderr, flush=True)
    out["s16_mono_11025"] = shape
    del pinned, wins
    # 48 kHz planar-float stereo (pageable: numpy arrays), against run_pcm_format with the window at the whole stream
    rate = 48000
    planes = []
    for e in eps:
        mono = e.pcm[: len(e.pcm) // 2]
        idx = (np.arange(int(len(mono) * rate / 11025), dtype=np.int64) * 11025) // rate
        left = mono[idx].astype(np.float32) / np.float32(32768.0)
        planes.append([left, np.ascontiguousarray(left * np.float32(0.5))])
    an = capi.Analyzer.from_files([f"ep{k}.wav" for k in range(len(eps))]).with_opening_search_percentage(1.0)
    shape = {"chunks": {}}
    for name, secs in [("0.5s", 0.5), ("5s", 5.0), ("60s", 60.0)]:
        chunk = int(secs * rate)
        one, fed = [], []
        for _ in range(repeats):
            one.append(median_ms(lambda: an.run_pcm(planes, channels=2, sample_rate=rate, sample_format=capi.SAMPLE_F32P), 1))
            fed.append(median_ms(lambda: feed_all(planes, 2, rate, capi.SAMPLE_F32P, chunk, True), 1))
        shape["chunks"][name] = {"fed_ms": statistics.median(fed), "one_shot_ms": statistics.median(one),
                                 "feeds": -(-len(planes[0][0]) // chunk)}
        print("f32p stereo 48000", name, shape["chunks"][name], file=sys.stderr, flush=True)
    out["f32p_stereo_48000"] = shape
    return out


def bench_per_feed():
    rng = np.random.default_rng(1)
    second = rng.integers(-20000, 20000, 11025, dtype=np.int16)
    out = {}
    for lanes in (1, 28, 256):
        f = capi.Feeder(lanes, 1, 11025, capi.SAMPLE_S16, 2)
        chunks = [second] * lanes
        for _ in range(5):
            f.feed(chunks)
        f.ready(0)
        times = []
        for _ in range(60):
            t0 = time.perf_counter()
            f.feed(chunks)
            f.ready(0)                                   # the feed's items are on the host
            times.append((time.perf_counter() - t0) * 1e3)
        out[str(lanes)] = {"ms_per_feed": statistics.median(times)}
    return out


def bench_state():
    """What a lane really carried (state_bytes[0] is the carry's high-water) over ten minutes of 1-s chunks."""
    out = {}
    for name, ch, rate, fmt, dtype in [("s16_mono_11025", 1, 11025, capi.SAMPLE_S16, np.int16), ("s16_stereo_11025", 2, 11025, capi.SAMPLE_S16, np.int16),
                                       ("f32p_stereo_48000", 2, 48000, capi.SAMPLE_F32P, np.float32), ("f32p_6ch_48000", 6, 48000, capi.SAMPLE_F32P, np.float32),
                                       ("s16_stereo_44100", 2, 44100, capi.SAMPLE_S16, np.int16)]:
        rng = np.random.default_rng(2)
        planar = fmt == capi.SAMPLE_F32P
        if planar:
            chunk = [[rng.uniform(-0.5, 0.5, rate).astype(dtype) for _ in range(ch)]]
        else:
            chunk = [rng.integers(-20000, 20000, rate * ch, dtype=dtype)]
        f = capi.Feeder(1, ch, rate, fmt, 2)
        for _ in range(600):
            f.feed(chunk)
        f.ready(0)
        out[name] = f.state_bytes()[0]
    return out


def trace_child(lanes, feeds):
    second = np.random.default_rng(1).integers(-20000, 20000, 11025, dtype=np.int16)
    f = capi.Feeder(lanes, 1, 11025, capi.SAMPLE_S16, 2)
    for _ in range(feeds):
        f.feed([second] * lanes)
    f.finish()
    f.ready(0)


def bench_launches(feeds):
    """Kernel calls per feed from rocprofv3's statistics of a child process that does nothing but feed."""
    if not shutil.which("rocprofv3"):
        return NOT_MEASURED
    out = {}
    for lanes in (1, 28, 256):
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
                   sys.executable, os.path.abspath(__file__), "--trace-child", str(lanes), "--trace-feeds", str(feeds)]
            run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
            stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if run.returncode != 0 or not stats:
                print(run.stdout[-2000:], file=sys.stderr)
                return NOT_MEASURED
            calls = {}
            for path in stats:
                for row in csv.DictReader(open(path)):
                    name = row["Name"].replace("needle::(anonymous namespace)::", "").replace("needle::stft::", "").replace("void ", "")
                    name = re.sub(r"\(.*", "", name)   # (the argument list; after the namespaces, which hold a parenthesis too)
                    calls[name] = calls.get(name, 0) + int(row["Calls"])
            # feeds + the finish round
            out[str(lanes)] = {"rounds": feeds + 1, "calls": calls, "per_feed": round(sum(calls.values()) / (feeds + 1), 2)}
    return out


RESOURCE_FILES = ["feeder.hip", "fingerprint.hip", "fingerprint32.hip", "convert.hip", "downmix.hip"]
RESOURCE_KERNELS = re.compile(r"feeder_carry_kernel|stft_chroma32_kernel|features_classify|stft_chroma_kernel|fixup_items_kernel|audit_items_kernel"
                              r"|feeder_ingest_kernel|convert_kernel|downmix_kernel")
RESOURCE_KEYS = {"TotalSGPRs": "sgprs", "SGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
                 "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}


def kernel_resources(root):
    """{kernel: {sgprs, vgprs, agprs, scratch, occupancy, lds}} of a tree's feeder and fingerprint kernels, compiled for
    gfx950 with the flags of needle_amd/csrc/Makefile (device side only, nothing is written)."""
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
    names = dict(zip(mangled, mangled))
    if shutil.which("c++filt") and mangled:
        plain = subprocess.run(["c++filt", "-p"], input="\n".join(mangled), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
        names = {m: p.replace("needle::(anonymous namespace)::", "").replace("needle::stft::", "").replace("void ", "") for m, p in zip(mangled, plain)}
    return {names[m]: v for m, v in out.items() if RESOURCE_KERNELS.search(names[m])}


def bench_resources(root, parent):
    this = kernel_resources(root)
    if not parent:
        return {"how": "hipcc -Rpass-analysis=kernel-resource-usage, gfx950", "kernels": {k: {"this": v} for k, v in sorted(this.items())}}
    before = kernel_resources(parent)

    def earlier(name):  # the same kernel in the parent: a template parameter added here with its default dropped
        for cand in (name, re.sub(r", false>$", ">", name), re.sub(r"<false>$", "", name)):
            if cand in before:
                return cand
        return None
    pairs = {k: earlier(k) for k in this}
    return {"how": "hipcc -Rpass-analysis=kernel-resource-usage on this tree and on the parent commit, gfx950",
            "unchanged": all(this[k] == before[b] for k, b in pairs.items() if b),
            "new": sorted(k for k, b in pairs.items() if not b),
            "gone": sorted(set(before) - set(pairs.values())),
            "kernels": {k: dict({"this": v}, **({"parent": before[pairs[k]], "parent_name": pairs[k]} if pairs[k] else {}))
                        for k, v in sorted(this.items())}}


def bench_headline(root, parent, repeats):
    def once(tree):
        run = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree,
                             stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=900, check=True)
        return json.loads(run.stdout.strip().splitlines()[-1])["value"]
    values = {"parent": [], "this": []}
    for _ in range(repeats):
        values["parent"].append(once(parent))
        values["this"].append(once(root))
        print("headline", values["parent"][-1], values["this"][-1], file=sys.stderr, flush=True)
    med = {k: statistics.median(v) for k, v in values.items()}
    return {"unit": "episode-pairs/s", "runs": values, "median": med,
            "difference_percent": round(100.0 * (med["this"] - med["parent"]) / med["parent"], 3),
            "spread_percent": {k: round(100.0 * (max(v) - min(v)) / med[k], 3) for k, v in values.items()}}


def audit_lanes(lanes=28, rate=48000):
    rng = np.random.default_rng(3)
    return [[rng.uniform(-0.5, 0.5, rate).astype(np.float32) for _ in range(2)] for _ in range(lanes)]


def timed_feed(f, chunks):
    t0 = time.perf_counter()
    f.feed(chunks)
    f.ready(0)                                           # the feed's items are on the host
    return (time.perf_counter() - t0) * 1e3


# The audit-off leg as a program of its own, run with a tree as its working directory so that it loads that tree's
# library: nothing in it is newer than the feeder itself.
AUDIT_LEG = """
import statistics, sys, time
import numpy as np
sys.path.insert(0, '.')
from needle_amd import capi
rng = np.random.default_rng(3)
chunks = [[rng.uniform(-0.5, 0.5, 48000).astype(np.float32) for _ in range(2)] for _ in range(28)]
f = capi.Feeder(28, 2, 48000, capi.SAMPLE_F32P, 2)
times = []
for k in range(40):
    t0 = time.perf_counter()
    f.feed(chunks)
    f.ready(0)
    times.append((time.perf_counter() - t0) * 1e3)
print(statistics.median(times[10:]))
"""


# bench_mixed's one_feeder leg as a program of its own, for the same purpose
MIXED_LEG = """
import statistics, sys, time
import numpy as np
sys.path.insert(0, '.')
from needle_amd import capi
rng = np.random.default_rng(4)
formats = [(6, 48000, capi.SAMPLE_F32P), (2, 44100, capi.SAMPLE_S16), (2, 48000, capi.SAMPLE_F32P), (1, 11025, capi.SAMPLE_S16)]
def second(ch, rate, fmt):
    if fmt == capi.SAMPLE_F32P:
        return [rng.uniform(-0.5, 0.5, rate).astype(np.float32) for _ in range(ch)]
    return rng.integers(-20000, 20000, rate * ch, dtype=np.int16)
chunks = [second(*fmt) for fmt in formats for _ in range(7)]
f = capi.Feeder.with_formats([fmt for fmt in formats for _ in range(7)], 2)
times = []
for k in range(40):
    t0 = time.perf_counter()
    f.feed(chunks)
    f.ready(0)
    times.append((time.perf_counter() - t0) * 1e3)
print(statistics.median(times[10:]))
"""


def uniform_vs_parent(root, parent, program=AUDIT_LEG):
    """The 28-lane 48 kHz planar-float stereo leg (or another program) in this tree and in the parent commit, five
    processes each, alternating."""
    def leg(tree):
        run = subprocess.run([sys.executable, "-c", program], cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                             text=True, timeout=300, check=True)
        return float(run.stdout.strip().splitlines()[-1])
    runs = {"parent": [], "this": []}
    for k in range(5):
        for name in (("parent", "this") if k % 2 == 0 else ("this", "parent")):
            runs[name].append(leg(parent if name == "parent" else root))
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = max(runs["parent"]) - min(runs["parent"])
    return {"unit": "ms per feed, median of 30 after 10, five processes each", "runs": runs, "median": med,
            "parent_spread": spread, "condition": "this <= parent + parent_spread", "holds": med["this"] <= med["parent"] + spread}


MIXED_FORMATS = [(6, 48000, capi.SAMPLE_F32P), (2, 44100, capi.SAMPLE_S16), (2, 48000, capi.SAMPLE_F32P), (1, 11025, capi.SAMPLE_S16)]


def bench_mixed():
    """28 lanes in four formats, 1-s chunks: through one with_formats feeder, and through four uniform feeders of seven
    lanes fed in turn.  Wall ms per feed of both (the items of the feed on the host), and the event times of the front
    end's kernels: ingest against convert + downmix."""
    rng = np.random.default_rng(4)

    def second(ch, rate, fmt):
        if fmt == capi.SAMPLE_F32P:
            return [rng.uniform(-0.5, 0.5, rate).astype(np.float32) for _ in range(ch)]
        return rng.integers(-20000, 20000, rate * ch, dtype=np.int16)
    groups = [[second(*fmt) for _ in range(7)] for fmt in MIXED_FORMATS]
    formats = [fmt for fmt in MIXED_FORMATS for _ in range(7)]
    one = capi.Feeder.with_formats(formats, 2)
    four = [capi.Feeder(7, ch, rate, fmt, 2) for ch, rate, fmt in MIXED_FORMATS]
    chunks = [c for g in groups for c in g]

    def feed_one():
        one.feed(chunks)
        one.ready(0)

    def feed_four():
        for f, g in zip(four, groups):
            f.feed(g)
        for f in four:
            f.ready(0)
    times = {"one_feeder": [], "four_feeders": []}
    for k in range(40):
        for name in (("one_feeder", "four_feeders") if k % 2 == 0 else ("four_feeders", "one_feeder")):
            t0 = time.perf_counter()
            (feed_one if name == "one_feeder" else feed_four)()
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = {"shape": "28 lanes, seven each of 5.1 planar-float 48 kHz, stereo s16 44.1 kHz, stereo planar-float 48 kHz, mono s16 11025 Hz; 1-s chunks, step 2",
           "ms_per_feed": {k: statistics.median(v[10:]) for k, v in times.items()}}
    kernels = ["ingest", "convert", "downmix", "resample", "feeder_carry", "stft_chroma32"]
    for name, fn in (("one_feeder", feed_one), ("four_feeders", feed_four)):
        capi.set_kernel_timing(",".join(kernels) + ",sum")
        for _ in range(30):
            fn()
        out.setdefault("kernel_ms_per_feed", {})[name] = {k: round(capi.last_kernel_ms(k) / 30, 5) for k in kernels if capi.last_kernel_ms(k) >= 0}
        out.setdefault("launches_per_feed", {})[name] = {k: capi.kernel_launches(k) / 30 for k in kernels if capi.kernel_launches(k)}
        capi.set_kernel_timing(None)
    for k in range(28):
        assert np.array_equal(one.items(k), four[k // 7].items(k % 7)), k
    out["state_bytes_per_lane"] = {"one_feeder": one.state_bytes()[0], "four_feeders": [f.state_bytes()[0] for f in four]}
    return out


def bench_switch(root, parent):
    out = {"uniform_vs_parent": uniform_vs_parent(root, parent) if parent else NOT_MEASURED,
           "mixed_vs_parent": uniform_vs_parent(root, parent, MIXED_LEG) if parent else NOT_MEASURED}
    rng = np.random.default_rng(6)
    a, b = (2, 48000, capi.SAMPLE_S16), (2, 44100, capi.SAMPLE_S16)
    chunk = {fmt: [rng.integers(-20000, 20000, fmt[1] * 2, dtype=np.int16) for _ in range(28)] for fmt in (a, b)}
    kernels = ["feeder_carry", "resample", "stft_chroma32", "features_cert", "stft_fallback", "fixup_items"]
    f = capi.Feeder.with_formats([a] * 28, 2)
    lanes = list(range(0, 28, 4))
    feeds, calls = [], []
    for sec in range(10):                                # every second: a feed, then the seven lanes switch (48 <-> 44.1 kHz)
        now = [f.lane_format(k) for k in range(28)]
        feeds.append(timed_feed(f, [chunk[fmt][k] for k, fmt in enumerate(now)]))
        to = b if now[0] == a else a
        capi.set_kernel_timing(",".join(kernels) + ",sum")
        t0 = time.perf_counter()
        f.switch_format(lanes, [to] * len(lanes))
        f.ready(0)
        wall = (time.perf_counter() - t0) * 1e3
        capi.synchronize()
        calls.append({"wall_ms": wall, "kernel_ms": round(sum(max(capi.last_kernel_ms(k), 0.0) for k in kernels), 5),
                      "launches": {k: capi.kernel_launches(k) for k in kernels if capi.kernel_launches(k)}})
        capi.set_kernel_timing(None)
    assert all(len(f.lane_segments(k)) == (11 if k in lanes else 1) for k in range(28))
    out["switch_call"] = {"shape": "28 lanes of 48 kHz s16 stereo, 1-s chunks, step 2; after every feed lanes 0, 4, ... 24 switch between 48 and 44.1 kHz",
                          "target": "none: recorded",
                          "feed_wall_ms_median": statistics.median(feeds[2:]),
                          "switch_wall_ms_median": statistics.median(c["wall_ms"] for c in calls[2:]),
                          "switch_kernel_ms_median": statistics.median(c["kernel_ms"] for c in calls[2:]),
                          "calls": calls}
    return out


def bench_audit(root, parent):
    chunks = audit_lanes()
    feeders = {}
    for on in (False, True):
        feeders[on] = capi.Feeder(len(chunks), 2, 48000, capi.SAMPLE_F32P, 2)
        feeders[on].set_audit(on)
    times = {False: [], True: []}
    for k in range(40):
        for on in ((False, True) if k % 2 == 0 else (True, False)):
            times[on].append(timed_feed(feeders[on], chunks))
    out = {"shape": "28 lanes, 48 kHz planar-float stereo, 1-s chunks, step 2",
           "ms_per_feed": {"audit_off": statistics.median(times[False][10:]), "audit_on": statistics.median(times[True][10:])}}
    a = feeders[True].audit()
    out["audit"] = a
    assert a["items"] == sum(feeders[True].ready(k)[0] for k in range(len(chunks))) and a["accepted_mismatches"] == 0
    kernels = ["stft_chroma32", "features_cert", "stft_fallback", "fixup_items", "audit_stft", "audit_items"]
    capi.set_kernel_timing(",".join(kernels) + ",sum")
    for _ in range(30):
        feeders[True].feed(chunks)
    feeders[True].ready(0)
    out["kernel_ms_per_feed"] = {k: round(capi.last_kernel_ms(k) / 30, 5) for k in kernels}
    capi.set_kernel_timing(None)
    out["state_bytes_per_lane"] = {"audit_off": feeders[False].state_bytes()[0], "audit_on": feeders[True].state_bytes()[0]}
    del feeders
    if parent:
        out["audit_off_vs_parent"] = uniform_vs_parent(root, parent)
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--episodes", type=int, default=28)
    ap.add_argument("--only", default="chunked,per_feed,state,launches,resources,headline,audit")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit (built, for the headline)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "feeder_bench.json"))
    ap.add_argument("--trace-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--trace-feeds", type=int, default=60)
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args.trace_child, args.trace_feeds)
    only = set(args.only.split(","))
    keys = ("device", "chunked", "per_feed", "state_bytes_per_lane", "kernel_launches_per_feed", "resources", "headline_vs_parent", "audit",
            "mixed", "uniform_vs_parent", "switch")
    res = {k: NOT_MEASURED for k in keys}
    if os.path.exists(args.out):                         # sections not run now keep their figures
        try:
            res.update({k: v for k, v in json.load(open(args.out)).items() if k in keys})
        except (OSError, ValueError):
            pass

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    if "resources" in only:
        res["resources"] = bench_resources(root, args.parent)
        save()
    if capi.device_count() > 0:
        res["device"] = capi.device_pci_bus_id()
        if "state" in only:
            res["state_bytes_per_lane"] = bench_state()
            save()
        if "per_feed" in only:
            res["per_feed"] = bench_per_feed()
            save()
        if "launches" in only:
            res["kernel_launches_per_feed"] = bench_launches(args.trace_feeds)
            save()
        if "chunked" in only:
            res["chunked"] = bench_chunked(args.episodes, max(args.repeats, 5))
            save()
        if "audit" in only:
            res["audit"] = bench_audit(root, args.parent)
            save()
        if "mixed" in only:
            res["mixed"] = bench_mixed()
            save()
        if "uniform" in only and args.parent:
            res["uniform_vs_parent"] = uniform_vs_parent(root, args.parent)
            save()
        if "switch" in only:
            res["switch"] = bench_switch(root, args.parent)
            save()
        if "headline" in only and args.parent:
            res["headline_vs_parent"] = bench_headline(root, args.parent, max(args.repeats, 3))
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
