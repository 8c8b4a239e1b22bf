"""Cost of 3-8 channel (surround) input: prints one JSON line.

  downmix   : the down-mix kernel alone on the opening windows of 28 x 24-min episodes of 6-channel 48 kHz PCM
              (0.97 G frames, 12 B read + 2 B written each), one launch through needle_hip_library_set_pcm_device; its
              event-timed duration and the achieved bytes/s as a share of the 6.29 TB/s float4 copy rate of the MI355X.
  run_pcm   : needle_hip_analyzer_run_pcm wall time from pinned host PCM (needle_hip_host_alloc), the same 48 kHz content
              as mono, stereo and 6 channels (upload + down-mix + resample + fingerprint of the opening windows).
  library   : ms per job (job_begin + job_end) of a resident 28 x 24 min library set from 6-channel PCM and from its
              down-mix as mono PCM (the resident PCM is then the same in both cases).

Usage: python tools/bench_multichannel.py [--steps K] [--warmup W] [--episodes N] [--analyzer-episodes M]
The kernel timer (event pairs around the launch) is separate from a profiler run: time this script on its own and
collect a kernel trace in another run."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from needle_amd import capi, synth  # noqa: E402

COPY_RATE = 6.29e12  # B/s, float4 copy measured on the MI355X


def bench_downmix(episodes, steps, warmup):
    ch, rate = 6, 48000
    frames = 24 * 60 * rate
    L = capi.lib()
    host = np.random.default_rng(1).integers(-32768, 32768, frames * ch, dtype=np.int16)
    bufs = []
    for _ in range(episodes):
        b = capi.DeviceBuffer(host.nbytes)
        capi.check(L.needle_hip_memcpy_h2d(b.ptr, host.ctypes.data, host.nbytes))
        bufs.append(b)
    del host
    lib = capi.Library(episodes)
    capi.set_kernel_timing("downmix")
    ms = []
    for k in range(warmup + steps):
        lib.set_pcm_device([b.ptr for b in bufs], [frames * ch] * episodes, channels=ch)
        if k >= warmup:
            ms.append(capi.last_kernel_ms("downmix"))
    capi.set_kernel_timing(None)
    window_frames = episodes * (frames // 2)
    nbytes = window_frames * (2 * ch + 2)
    med = statistics.median(ms)
    return {"episodes": episodes, "channels": ch, "frames": window_frames, "bytes": nbytes, "kernel_ms_median": med,
            "kernel_ms_min": min(ms), "bytes_per_s": nbytes / (med * 1e-3),
            "share_of_copy_rate": round(nbytes / (med * 1e-3) / COPY_RATE, 4)}


def bench_run_pcm(episodes, steps, warmup):
    rate = 48000
    eps = synth.make_library(episodes, 24 * 60.0, 90.0)
    mono48 = [np.repeat(e.pcm, 4)[: len(e.pcm) * rate // 11025] for e in eps]  # any 48 kHz content will do
    out = {}
    for ch in (1, 2, 6):
        pinned = []
        for k, m in enumerate(mono48):
            x = m if ch == 1 else np.repeat(m, 2) if ch == 2 else synth_surround(m, k)
            p = capi.PinnedArray(len(x))
            p.array[:] = x
            pinned.append(p)
        an = capi.Analyzer.from_files([f"e{k}.wav" for k in range(episodes)])
        t = []
        for k in range(warmup + steps):
            t0 = time.perf_counter()
            an.run_pcm([p.array for p in pinned], channels=ch, sample_rate=rate)
            if k >= warmup:
                t.append((time.perf_counter() - t0) * 1e3)
        out[f"c{ch}_ms"] = statistics.median(t)
        del pinned
    out["c6_over_c2"] = round(out["c6_ms"] / out["c2_ms"], 3)
    out["episodes"] = episodes
    return out


def synth_surround(mono, seed):
    from tests.test_multichannel_cpu import surround
    return surround(mono, 6, seed)


def bench_library(episodes, steps, warmup):
    eps = synth.make_library(episodes, 24 * 60.0, 90.0)
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(episodes)])
    out, results = {}, {}
    pcm6 = [synth_surround(e.pcm, k) for k, e in enumerate(eps)]
    mono = capi.downmix(pcm6, 6)  # the same resident content both ways: a job's cost depends on what it finds
    for ch in (1, 6):
        pcm = mono if ch == 1 else pcm6
        lib = capi.Library(episodes)
        lib.set_pcm(pcm, [len(p) for p in pcm], channels=ch)
        t = []
        for k in range(warmup + steps):
            t0 = time.perf_counter()
            lib.job_begin(cmp, 0)
            res, _ = lib.job_end(cmp, 0)
            if k >= warmup:
                t.append((time.perf_counter() - t0) * 1e3)
        out[f"c{ch}_ms_per_step"] = statistics.median(t)
        results[ch] = [None if r is None else (r.opening, r.ending) for r in res]
        del lib
    out["same_results"] = results[1] == results[6]
    out["episodes"] = episodes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=28)
    ap.add_argument("--analyzer-episodes", type=int, default=4)
    ap.add_argument("--only", choices=["downmix", "run_pcm", "library"], default=None)
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("needs a HIP device")
    res = {}
    if a.only in (None, "downmix"):
        res["downmix"] = bench_downmix(a.episodes, a.steps, a.warmup)
    if a.only in (None, "run_pcm"):
        res["run_pcm"] = bench_run_pcm(a.analyzer_episodes, max(a.steps // 2, 1), 1)
    if a.only in (None, "library"):
        res["library"] = bench_library(a.episodes, a.steps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
