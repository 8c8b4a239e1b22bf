"""Cost of a channel mix against the plain average it replaces: prints one JSON line.

The opening windows of 28 x 24-min episodes of 6-channel 48 kHz s16 PCM resident in HBM (0.97 G frames, 12 B read + 2 B
written each) go through needle_hip_library_set_pcm_device, one launch per call, four ways:

  downmix        interleaved s16, no mix: downmix.hip's kernel, what these bytes cost without a mix
  rematrix       interleaved s16 under the default 5.1 mix: rematrix.hip
  convert        planar s16, no mix: convert.hip with the plain down-mix fused in
  rematrix_p     planar s16 under the default 5.1 mix

Each is timed by the library's own event pairs (needle_hip_last_kernel_ms), `steps` runs after `warmup`; the JSON holds
every run, the median, the spread and the achieved bytes/s as a share of the 6.29 TB/s float4 copy rate of the MI355X.

Usage: python tools/bench_channel_mix.py [--steps K] [--warmup W] [--episodes N]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from needle_amd import capi  # noqa: E402

COPY_RATE = 6.29e12  # B/s, float4 copy measured on the MI355X
CH, RATE, MASK = 6, 48000, 0x60F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--episodes", type=int, default=28)
    a = ap.parse_args()
    frames = 24 * 60 * RATE
    L = capi.lib()
    host = np.random.default_rng(1).integers(-32768, 32768, frames * CH, dtype=np.int16)
    bufs = []
    for _ in range(a.episodes):
        b = capi.DeviceBuffer(host.nbytes)
        capi.check(L.needle_hip_memcpy_h2d(b.ptr, host.ctypes.data, host.nbytes))
        bufs.append(b)
    del host
    interleaved = [b.ptr for b in bufs]
    planes = [b.ptr + c * frames * 2 for b in bufs for c in range(CH)]      # the same bytes read as six planes
    mix = capi.channel_mix_default(MASK)
    window_frames = a.episodes * (frames // 2)
    nbytes = window_frames * (2 * CH + 2)
    res = {"episodes": a.episodes, "channels": CH, "frames": window_frames, "bytes": nbytes}
    for name, kernel, ptrs, fmt, m in [("downmix", "downmix", interleaved, capi.SAMPLE_S16, None),
                                       ("rematrix", "rematrix", interleaved, capi.SAMPLE_S16, mix),
                                       ("convert", "convert", planes, capi.SAMPLE_S16P, None),
                                       ("rematrix_p", "rematrix", planes, capi.SAMPLE_S16P, mix)]:
        lib = capi.Library(a.episodes).set_sample_format(fmt).set_channel_mix(m)
        capi.set_kernel_timing(kernel)
        ms = []
        for k in range(a.warmup + a.steps):
            lib.set_pcm_device(ptrs, [frames * CH] * a.episodes, channels=CH)
            if k >= a.warmup:
                ms.append(capi.last_kernel_ms(kernel))
        capi.set_kernel_timing(None)
        del lib
        med = statistics.median(ms)
        res[name] = {"kernel_ms": [round(v, 4) for v in ms], "median": round(med, 4), "min": round(min(ms), 4),
                     "max": round(max(ms), 4), "bytes_per_s": nbytes / (med * 1e-3),
                     "share_of_copy_rate": round(nbytes / (med * 1e-3) / COPY_RATE, 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
