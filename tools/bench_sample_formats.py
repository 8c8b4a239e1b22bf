"""Cost of PCM in the decoder's sample format (needle_hip_library_set_sample_format): prints one JSON line.

  kernel  : the conversion kernel alone on the opening windows of 28 x 24-min episodes of 48 kHz PCM resident in HBM, one
            launch through needle_hip_library_set_pcm_device (the library is told 11025 Hz so that the kernel writes
            straight into the resident PCM and nothing else runs): F32 stereo interleaved, F32P stereo, F32P 6-channel
            (down-mix fused, mono out) and S32 stereo.  Event-timed medians, bytes read + written over time, and that as a
            share of the 6.29 TB/s float4 copy rate of the MI355X (tools/bench_multichannel.py's yardstick).
  set_pcm : needle_hip_library_set_pcm wall time from pageable host memory, 48 kHz stereo, the same content as S16, F32
            and F32P, in one run; beside it what a caller without the feature does: numpy (one thread) converts the
            opening windows to s16, then the S16 set_pcm.
  job     : ms per job (job_begin + job_end) of the S16 and the F32 library after set_pcm (the resident PCM is the same).

Usage: python tools/bench_sample_formats.py [--steps K] [--warmup W] [--episodes N] [--upload-episodes M] [--out FILE]
The kernel timer (event pairs around the launch) is separate from a profiler run: time this script on its own and
collect a kernel trace in another run (--only kernel)."""
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
RATE = 48000

# name -> (format, channels, bytes read per frame, bytes written per frame)
KERNEL_SHAPES = {
    "f32_stereo": (capi.SAMPLE_F32, 2, 8, 4),
    "f32p_stereo": (capi.SAMPLE_F32P, 2, 8, 4),
    "f32p_6ch_fused": (capi.SAMPLE_F32P, 6, 24, 2),
    "s32_stereo": (capi.SAMPLE_S32, 2, 8, 4),
}


def bench_kernel(episodes, steps, warmup, only=None):
    frames = 24 * 60 * RATE
    L = capi.lib()
    out = {}
    for name, (fmt, ch, rd, wr) in KERNEL_SHAPES.items():
        if only and name not in only:
            continue
        planar = capi.sample_format_planar(fmt)
        dtype = capi.sample_format_dtype(fmt)
        plane_samples = frames if planar else frames * ch
        rng = np.random.default_rng(1)
        host = (rng.random(plane_samples, dtype=np.float32) * 2 - 1) if dtype == np.float32 else \
            rng.integers(-2 ** 31, 2 ** 31, plane_samples, dtype=np.int64).astype(np.int32)
        bufs = []
        for _ in range(episodes * (ch if planar else 1)):
            b = capi.DeviceBuffer(host.nbytes)
            capi.check(L.needle_hip_memcpy_h2d(b.ptr, host.ctypes.data, host.nbytes))
            bufs.append(b)
        del host
        lib = capi.Library(episodes).set_sample_format(fmt)
        capi.set_kernel_timing("convert")
        ms = []
        for k in range(warmup + steps):
            lib.set_pcm_device([b.ptr for b in bufs], [frames * ch] * episodes, channels=ch)
            if k >= warmup:
                ms.append(capi.last_kernel_ms("convert"))
        capi.set_kernel_timing(None)
        del lib, bufs
        window_frames = episodes * (frames // 2)
        nbytes = window_frames * (rd + wr)
        med = statistics.median(ms)
        out[name] = {"episodes": episodes, "channels": ch, "frames": window_frames, "bytes": nbytes,
                     "kernel_ms_median": med, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
                     "bytes_per_s": nbytes / (med * 1e-3), "share_of_copy_rate": round(nbytes / (med * 1e-3) / COPY_RATE, 4)}
    return out


def host_to_s16(x):
    """What a caller does today: rint(x * 32768), clipped, as int16 (numpy, one thread)."""
    return np.clip(np.rint(x * np.float32(32768.0)), -32768, 32767).astype(np.int16)


def bench_set_pcm_and_job(episodes, steps, warmup):
    ch = 2
    eps = synth.make_library(episodes, 24 * 60.0, 90.0)
    s16 = [np.repeat(np.repeat(e.pcm, 4)[: len(e.pcm) * RATE // 11025], 2) for e in eps]  # any 48 kHz stereo content will do
    del eps
    f32 = [p.astype(np.float32) / np.float32(32768.0) for p in s16]                       # exact: the same resident PCM
    f32p = [[np.ascontiguousarray(x[c::ch]) for c in range(ch)] for x in f32]
    lens = [len(p) for p in s16]
    cmp = capi.Comparator([f"ep{k}.wav" for k in range(episodes)])
    inputs = {"s16": (None, s16), "f32": (capi.SAMPLE_F32, f32), "f32p": (capi.SAMPLE_F32P, f32p)}
    times = {k: [] for k in inputs}
    times["host_convert_then_s16"] = []
    host_convert = []
    libs = {}
    for k in range(warmup + steps):                                                        # interleaved: same conditions for all
        for name, (fmt, pcm) in inputs.items():
            lib = capi.Library(episodes).set_sample_rate(RATE)
            if fmt is not None:
                lib.set_sample_format(fmt)
            t0 = time.perf_counter()
            lib.set_pcm(pcm, lens, channels=ch)
            if k >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
            libs[name] = lib
        lib = capi.Library(episodes).set_sample_rate(RATE)
        t0 = time.perf_counter()
        converted = [host_to_s16(x[: len(x) // ch // 2 * ch + 16 * ch]) for x in f32]      # the opening windows only
        t1 = time.perf_counter()
        # (the converted windows stand in for the streams: set_pcm is given the full lengths and reads the windows)
        lib.set_pcm(converted, lens, channels=ch)
        if k >= warmup:
            host_convert.append((t1 - t0) * 1e3)
            times["host_convert_then_s16"].append((time.perf_counter() - t0) * 1e3)
        del lib, converted
    window_values = sum(n // ch // 2 * ch for n in lens)
    out = {"episodes": episodes, "channels": ch, "rate": RATE, "window_values": window_values,
           "host_convert_ms": statistics.median(host_convert)}
    for name, t in times.items():
        out[f"{name}_ms"] = statistics.median(t)
        out[f"{name}_ms_min_max"] = [min(t), max(t)]
    out["f32_over_s16"] = round(out["f32_ms"] / out["s16_ms"], 3)
    out["f32p_over_s16"] = round(out["f32p_ms"] / out["s16_ms"], 3)
    out["f32_gb_per_s"] = round(window_values * 4 / (out["f32_ms"] * 1e-3) / 1e9, 2)
    out["s16_gb_per_s"] = round(window_values * 2 / (out["s16_ms"] * 1e-3) / 1e9, 2)
    job, results = {}, {}
    t = {name: [] for name in ("s16", "f32")}
    for k in range(warmup + steps):
        for name in t:
            t0 = time.perf_counter()
            libs[name].job_begin(cmp, 0)
            res, _ = libs[name].job_end(cmp, 0)
            if k >= warmup:
                t[name].append((time.perf_counter() - t0) * 1e3)
            results[name] = [None if r is None else (r.opening, r.ending) for r in res]
    for name in t:
        job[f"{name}_ms_per_job"] = statistics.median(t[name])
        job[f"{name}_ms_min_max"] = [min(t[name]), max(t[name])]
    job["same_results"] = results["s16"] == results["f32"]
    job["matched"] = sum(r is not None and r[0] is not None for r in results["f32"])
    job["episodes"] = episodes
    return out, job


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=28)
    ap.add_argument("--upload-episodes", type=int, default=8)
    ap.add_argument("--only", choices=["kernel", "set_pcm"], default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated kernel shapes (default: all)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("needs a HIP device")
    res = {}
    if a.only in (None, "kernel"):
        res["kernel"] = bench_kernel(a.episodes, a.steps, a.warmup, a.shapes.split(",") if a.shapes else None)
    if a.only in (None, "set_pcm"):
        res["set_pcm"], res["job"] = bench_set_pcm_and_job(a.upload_episodes, max(a.steps // 2, 2), 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
