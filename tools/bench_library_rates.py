#!/usr/bin/env python3
"""Cost of library PCM at decode rates (needle_hip_library_set_sample_rate): prints one JSON line and writes it to
profiles/library_rates_bench.json (--out).

The same content -- configs[1]'s 28 x 24 min episodes, 90 s shared intro -- as 11025 Hz mono, 44.1 kHz stereo, 48 kHz
stereo and 48 kHz 6-channel PCM.  Per form:
  set_pcm_ms        : needle_hip_library_set_pcm wall time from pageable host PCM (upload, down-mix, resample)
  set_pcm_device_ms : needle_hip_library_set_pcm_device wall time from device buffers 2 bytes off a 16-byte boundary
  stream_pcm_ms     : needle_hip_library_stream_pcm wall time (upload + down-mix + resample + fingerprint overlapped)
  job_ms            : ms per job (job_begin + job_end) after set_pcm; the resident PCM is 11025 Hz mono in every form
Only the opening windows (the first half of every stream) are materialised on the host: the library reads nothing
else, and num_values still gives the whole streams' lengths.

Usage: python tools/bench_library_rates.py [--steps K] [--warmup W] [--episodes N] [--forms 48000x2,...] [--out PATH]
The kernel times come from a separate rocprofv3 --kernel-trace --stats run of this script (one step, no warm-up)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from needle_amd import capi, synth  # noqa: E402

FORMS = ["11025x1", "44100x2", "48000x2", "48000x6"]


def opening_half(mono, rate, ch):
    """The first half (plus two frames) of an 11025 Hz mono episode brought to `rate` by sample-and-hold, in `ch`
    channels that differ, and the whole stream's length in values."""
    frames = len(mono) * rate // 11025
    keep = frames // 2 + 2
    up = mono[(np.arange(keep, dtype=np.int64) * 11025) // rate]
    if ch == 1:
        return up, frames
    x = up.astype(np.int32)
    chans = [up, (x >> 1).astype(np.int16), (x - (x >> 2)).astype(np.int16), (x >> 3).astype(np.int16),
             (-x // 3).astype(np.int16), (x // 5).astype(np.int16)][:ch]
    return np.stack(chans, axis=1).reshape(-1), frames * ch


def wall(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=28)
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "library_rates_bench.json"))
    a = ap.parse_args()
    eps = synth.make_library(a.episodes, 24 * 60.0, 90.0)
    n = len(eps)
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(n)])
    L = capi.lib()
    out = {"episodes": n, "minutes": 24, "steps": a.steps, "warmup": a.warmup, "forms": {}}
    for form in a.forms.split(","):
        rate, ch = (int(x) for x in form.split("x"))
        pcms, lens = zip(*[opening_half(e.pcm, rate, ch) for e in eps])
        r = {"rate": rate, "channels": ch, "host_bytes_read": 0}
        lib = capi.Library(n).set_sample_rate(rate)
        r["set_pcm_ms"] = wall(lambda: lib.set_pcm(pcms, lens, channels=ch))
        for _ in range(a.warmup):
            lib.job_begin(cmp, 0)
            lib.job_end(cmp, 0)
        times = []
        for _ in range(a.steps):
            t = time.perf_counter()
            lib.job_begin(cmp, 0)
            res, _ = lib.job_end(cmp, 0)
            times.append((time.perf_counter() - t) * 1e3)
        r["job_ms"] = statistics.median(times) if times else None
        r["job_ms_min"] = min(times) if times else None
        r["openings_found"] = sum(x is not None and x.opening is not None for x in res) if times else None
        del lib
        if a.steps:
            bufs, ptrs = [], []
            for p in pcms:
                b = capi.DeviceBuffer(p.nbytes + 16)
                capi.check(L.needle_hip_memcpy_h2d(b.ptr + 2, p.ctypes.data, p.nbytes))
                bufs.append(b)
                ptrs.append(b.ptr + 2)
            dev = capi.Library(n).set_sample_rate(rate)
            r["set_pcm_device_ms"] = wall(lambda: dev.set_pcm_device(ptrs, lens, channels=ch))
            del dev, bufs
        st = capi.Library(n).set_sample_rate(rate)
        r["stream_pcm_ms"] = wall(lambda: st.stream_pcm(pcms, lens, channels=ch))
        del st
        # what set_pcm reads from the host: the opening windows
        r["host_bytes_read"] = int(sum(2 * ch * ((ln // ch) * 1 // 2) for ln in lens))
        out["forms"][form] = r
        del pcms
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
