"""Libraries that differ in everything the library job pipeline shares, and the schedule that puts them in flight side by
side, for tests/test_gpu_pipeline.py.  Run as a child process (one per pipeline mode: the library and first-pass streams
are created once per process, so NEEDLE_HIP_STFT_SHARE and NEEDLE_HIP_LIBRARY_PRIORITY only take effect in a fresh one):

  python tests/pipeline_worker.py <out.json>

rebuilds libraries A, B, D and H from their seeds, runs SCHEDULE with H in the third role, and writes every job's results,
sorted run list and the arena's hashes.  With NEEDLE_HIP_TRACE set, it writes a marker line to stderr in front of every
job_begin, so that the parent can tell which job's first pass ran beside the other pipe.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from needle_amd import capi, synth  # noqa: E402

SEED_C = 0x5EC0DC
SEED_D = 0xD0D0D0
HOSTILE_SAMPLES = int(6 * 60 * synth.RATE)


class Spec:
    """One library of the pipeline tests: its PCM (host), how it is built, and the comparator its jobs run."""

    def __init__(self, name, pcm, channels, hash_duration, endings=False, opening=None, min_s=10, device=None):
        self.name, self.pcm, self.channels, self.hash_duration = name, pcm, channels, hash_duration
        self.endings, self.opening, self.min_s, self.device = endings, opening, min_s, device
        self.n = len(pcm)

    def library(self):
        kw = {} if self.opening is None else {"opening_search_percentage": self.opening}
        lib = capi.Library(self.n, hash_duration=self.hash_duration, **kw)
        if self.endings:
            lib.include_endings()
        if self.device is not None:
            lib.set_pcm_device(self.device.pointers(), [len(p) for p in self.pcm])
        else:
            lib.set_pcm(self.pcm, [len(p) for p in self.pcm], channels=self.channels)
        return lib

    def comparator(self):
        return capi.Comparator([f"{self.name}{k}.wav" for k in range(self.n)], include_endings=self.endings,
                               min_opening_duration=self.min_s, min_ending_duration=self.min_s)


def spec_a():
    """7 mono episodes of 90 s, hash_duration 0.3 s (step 2), openings only."""
    return Spec("a", [e.pcm for e in synth.make_library(7, 90.0, 25.0)], 1, 0.3)


def spec_b():
    """5 stereo episodes of 70 .. 130 s (a little channel difference), hash_duration 0.5 s (step 4), endings on."""
    rng = np.random.default_rng(41)
    pcm = []
    for k in range(5):
        e = synth.make_episode(k, 70.0 + 15.0 * k, 22.0, 21.0, seed_base=synth.EPISODE_SEED ^ 0xB)
        s = np.repeat(e.pcm, 2)
        s[1::2] = np.clip(s[1::2].astype(np.int32) + rng.integers(-3, 4, len(e.pcm)), -32768, 32767)
        pcm.append(s)
    return Spec("b", pcm, 2, 0.5, endings=True)


def spec_c():
    """A's geometry (same count, same lengths), other PCM."""
    return Spec("c", [e.pcm for e in synth.make_library(7, 90.0, 25.0, seed_base=SEED_C)], 1, 0.3)


def opening_samples(samples):
    """The opening window of a stream of `samples` frames at the default 50 %: duration and product in f32 nanoseconds,
    as the reference's analyzer computes it (one sample short of samples // 2 for some lengths)."""
    from oracle import oracle as O
    dur = O.duration_from_secs_f64(samples * (1.0 / 11025.0))
    return O.duration_mul_f32(dur, 0.5) * 11025 // O.NS


def d_samples(kept_a):
    """An episode length (samples) whose opening window holds exactly `kept_a` hashes at step 4, away from both edges."""
    from oracle import oracle as O
    total = 2 * (4096 + 1365 * (4 * (kept_a - 1) + 20))       # raw items 4 (kept_a - 1) + 2 of 4 (kept_a - 1) + 1 .. 4 kept_a
    assert -(-O.num_items(opening_samples(total)) // 4) == kept_a
    return total


def spec_d(kept_a):
    """A's video count, rows exactly as long as A's, hash_duration 0.5 s: same row-table sizes, other timestamps."""
    total = d_samples(kept_a)
    return Spec("d", [e.pcm for e in synth.make_library(7, total / synth.RATE, 40.0, seed_base=SEED_D)], 1, 0.5)


def spec_h():
    """8 hostile windows of 6 minutes (silence, sustained chords), generated on the device, whole stream searched."""
    gen = synth.DeviceLibrary(8, HOSTILE_SAMPLES, 40.0, hostile=True)
    return Spec("h", [gen.episode(k) for k in range(8)], 1, 0.3, opening=1.0, min_s=20, device=gen)


# The fixed schedule: roles P (the main library), Q (other geometry), R (P's geometry or a large one), S (P's row-table
# sizes).  Every round: P beside Q in both slot orders, ends in both orders, two libraries on one slot (one pipe, one
# epilogue workspace) with either ending first, three jobs in flight on two pipes.
ROUND = [
    ("b", "P", 0), ("b", "Q", 1), ("e", "P", 0), ("e", "Q", 1),
    ("b", "Q", 0), ("b", "P", 1), ("e", "P", 1), ("e", "Q", 0),
    ("b", "P", 0), ("b", "R", 0), ("e", "R", 0), ("e", "P", 0),
    ("b", "S", 0), ("b", "P", 0), ("e", "S", 0), ("e", "P", 0),
    ("b", "P", 0), ("b", "Q", 1), ("b", "R", 0), ("e", "Q", 1), ("e", "P", 0), ("e", "R", 0),
    ("b", "S", 0), ("b", "R", 1), ("e", "R", 1), ("b", "P", 1), ("e", "S", 0), ("e", "P", 1),
]
ROUNDS = 3


def run_schedule(libs, cmps, roles, on_end, marker=None):
    """libs / cmps: name -> Library / Comparator; roles: role -> name.  on_end(name, slot, lib, results, found) after every
    job_end; marker(name, slot) in front of every job_begin."""
    for _ in range(ROUNDS):
        for op, role, slot in ROUND:
            name = roles[role]
            if op == "b":
                if marker:
                    marker(name, slot)
                libs[name].job_begin(cmps[name], slot)
            else:
                res, found = libs[name].job_end(cmps[name], slot)
                on_end(name, slot, libs[name], res, found)


def arena_rows(lib, spec):
    """Every row of the library's hash arena, cut to its kept length (the lengths come from frame_hashes)."""
    d_arena, stride = lib.hash_arena()
    R = lib.rows_per_video()
    arena = np.zeros(spec.n * R * stride, dtype=np.uint32)
    capi.check(capi.lib().needle_hip_memcpy_d2h(arena.ctypes.data, d_arena, arena.nbytes))
    arena = arena.reshape(spec.n * R, stride)
    rows = []
    for v in range(spec.n):
        fh = lib.frame_hashes(v)
        regions = [len(fh.opening_data()[0])] + ([len(fh.ending_data()[0])] if R > 1 else [])
        rows.append([arena[v * R + r, :k].tolist() for r, k in enumerate(regions)])
    return rows


def sorted_runs(runs):
    keys = np.stack([runs[f].astype(np.int64) for f in capi.RUN_DTYPE.names], axis=1).reshape(-1, 6)
    return keys[np.lexsort(keys.T[::-1])]


def main(out):
    specs = {"a": spec_a(), "b": spec_b(), "h": spec_h()}
    kept_a = int(capi.lib().needle_hip_fingerprint_num_kept(opening_samples(len(specs["a"].pcm[0])), 2))
    specs["d"] = spec_d(kept_a)
    libs = {k: s.library() for k, s in specs.items()}
    specs["h"].device.free()
    cmps = {k: s.comparator() for k, s in specs.items()}
    jobs = []

    def on_end(name, slot, lib, res, found):
        jobs.append({"lib": name, "slot": slot, "found": int(found),
                     "results": [None if r is None else [r.opening, r.ending] for r in res],
                     "runs": sorted_runs(lib.job_runs(slot)).tolist(), "rows": arena_rows(lib, specs[name])})

    def marker(name, slot):
        sys.stderr.flush()
        os.write(2, f"[pipeline_worker] job_begin {name} {slot}\n".encode())

    run_schedule(libs, cmps, {"P": "a", "Q": "b", "R": "h", "S": "d"}, on_end,
                 marker if os.environ.get("NEEDLE_HIP_TRACE") else None)
    with open(out, "w") as f:
        json.dump({"jobs": jobs}, f)


if __name__ == "__main__":
    main(sys.argv[1])
