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

--mixed: ONE library whose videos cycle through the forms (needle_hip_library_set_video_formats; the 6-channel ones
under the default mix of mask 0x3F), written to profiles/library_formats_bench.json:
  mixed.set_pcm_ms / stream_pcm_ms : the mixed season through one call (median of --steps calls after --warmup, a fresh
                                     library each)
  uniform_sum.*                    : the same videos as one uniform library per form, each form's median, added up
  landing                          : the landing launches of one mixed set_pcm -- their kernel time, the bytes they read
                                     and write, and their rate, to hold against the device-copy figure in DESIGN.md
  landing_device                   : the same for set_pcm_device from device buffers that start on a 16-byte boundary
                                     and from buffers one sample past it (the landing kernel's scalar path)
  launches                         : landing and resampler launches of the mixed set_pcm

Usage: python tools/bench_library_rates.py [--steps K] [--warmup W] [--episodes N] [--forms 48000x2,...] [--mixed] [--out PATH]
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


def mixed(a):
    """One season cycling through the forms against one uniform library per form."""
    forms = [tuple(int(x) for x in form.split("x")) for form in a.forms.split(",")]
    eps = synth.make_library(a.episodes, 24 * 60.0, 90.0)
    n = len(eps)
    form_of = [forms[k % len(forms)] for k in range(n)]
    pcms, lens = zip(*[opening_half(e.pcm, rate, ch) for e, (rate, ch) in zip(eps, form_of)])
    del eps
    formats = [(ch, rate, capi.SAMPLE_S16) for rate, ch in form_of]
    mixes = [capi.channel_mix_default(0x3F) if ch == 6 else None for _, ch in form_of]
    out = {"episodes": n, "minutes": 24, "forms": a.forms.split(","), "mixed": {}, "uniform_sum": {}}

    out["steps"], out["warmup"] = a.steps, a.warmup

    def library():
        return capi.Library(n).set_video_formats(formats, mixes)

    def median_ms(make, call):
        """Median wall time of `call` on a fresh library, --steps times after --warmup."""
        times = []
        for k in range(a.warmup + a.steps):
            lib = make()
            t = wall(lambda: call(lib))
            if k >= a.warmup:
                times.append(t)
            del lib
        return statistics.median(times)
    out["mixed"]["set_pcm_ms"] = median_ms(library, lambda lib: lib.set_pcm(pcms, lens, channels=0))
    out["mixed"]["stream_pcm_ms"] = median_ms(library, lambda lib: lib.stream_pcm(pcms, lens, channels=0))
    lib = library()
    lib.set_pcm(pcms, lens, channels=0)
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(n)])
    lib.job_begin(cmp, 0)
    res, _ = lib.job_end(cmp, 0)
    out["mixed"]["openings_found"] = sum(x is not None and x.opening is not None for x in res)
    del lib
    landing = "rematrix" if any(m is not None for m in mixes) else "ingest"
    read = sum(p.nbytes for p in pcms)
    written = sum(2 * (len(p) // ch) for p, (_, ch) in zip(pcms, form_of))

    def landing_of(call):
        capi.set_kernel_timing(f"{landing},resample,sum")
        timed = library()
        call(timed)
        ms = capi.last_kernel_ms(landing)
        launches = {k: capi.kernel_launches(k) for k in (landing, "resample")}
        capi.set_kernel_timing(None)
        del timed
        return {"kernel": landing, "ms": ms, "bytes_read": int(read), "bytes_written": int(written),
                "gb_per_s": (read + written) / ms / 1e6 if ms else None}, launches
    out["landing"], out["launches"] = landing_of(lambda lib: lib.set_pcm(pcms, lens, channels=0))
    L = capi.lib()
    out["landing_device"] = {}
    for name, off in (("aligned", 0), ("one_sample_off", 2)):
        bufs, ptrs = [], []
        for p in pcms:
            b = capi.DeviceBuffer(p.nbytes + 32)
            at = (b.ptr + 15) // 16 * 16 + off
            capi.check(L.needle_hip_memcpy_h2d(at, p.ctypes.data, p.nbytes))
            bufs.append(b)
            ptrs.append(at)
        library().set_pcm_device(ptrs, lens, channels=0)
        out["landing_device"][name], _ = landing_of(lambda lib: lib.set_pcm_device(ptrs, lens, channels=0))
        del bufs
    sums = {"set_pcm_ms": 0.0, "stream_pcm_ms": 0.0}
    for rate, ch in forms:
        idx = [k for k in range(n) if form_of[k] == (rate, ch)]
        if not idx:
            continue
        sub, sub_lens = [pcms[k] for k in idx], [lens[k] for k in idx]

        def uniform():
            u = capi.Library(len(idx)).set_sample_rate(rate)
            return u.set_channel_mix(capi.channel_mix_default(0x3F)) if ch == 6 else u
        sums["set_pcm_ms"] += median_ms(uniform, lambda u: u.set_pcm(sub, sub_lens, channels=ch))
        sums["stream_pcm_ms"] += median_ms(uniform, lambda u: u.stream_pcm(sub, sub_lens, channels=ch))
    out["uniform_sum"] = sums
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=28)
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--mixed", action="store_true", help="one library with a format per video against one library per form")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "library_formats_bench.json" if a.mixed else "library_rates_bench.json")
    if a.mixed:
        line = json.dumps(mixed(a))
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
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
