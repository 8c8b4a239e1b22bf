"""-m gpu: a grouped search (Comparator.run_with_frame_hashes(groups=...): only videos of equal label are compared; the
numbering: needle_amd/csrc/pair_ids.h, the device epilogue under it: GroupedPairs / GroupedVideos in epilogue_kernels.h)
against the ORACLE's run_with_frame_hashes over every group's own sub-list.  Every case runs with the host epilogue
(NEEDLE_HIP_DEVICE_EPILOGUE=0) and with the device's (=1).  Hashes are planted as tests/test_gpu_epilogue.py plants them: rows
of a few hundred random hashes with shared segments written in; 246 ms a hash, minimum durations of 5-20 s, so runs of 21 and
more hashes qualify."""
import os
import subprocess

import numpy as np
import pytest

from needle_amd import capi, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
NS = O.NS
HD = O.duration_from_secs_f32(0.3)
STEP = 246_000_000
FORMS = ("0", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() > 0, "GPU tests need a HIP device (the product has no CPU fallback)"


def _as(rs):
    return [None if r is None else (r.opening, r.ending) for r in rs]


def members_of(labels):
    out = {}
    for v, g in enumerate(labels):
        out.setdefault(g, []).append(v)
    return list(out.values())


def random_rows(rng, lens, regions=1):
    return [[rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32) for _ in range(regions)] for k in lens]


def even_timestamps(rows, t0=2_600_000_000, step=STEP):
    return [[[t0 + 7_000 * NS * r + i * step for i in range(len(row))] for r, row in enumerate(video)] for video in rows]


class Videos:
    """Hash rows and timestamps as the product's FrameHashes and as the oracle's."""

    def __init__(self, rows, ts, paths=None):
        self.rows, self.ts, self.n = rows, ts, len(rows)
        self.endings = len(rows[0]) == 2
        self.paths = paths or [f"v{k}.mkv" for k in range(self.n)]
        pairs = lambda v, r: list(zip(rows[v][r].tolist(), ts[v][r]))
        self.c = [capi.FrameHashes.new(pairs(v, 0), pairs(v, 1) if self.endings else [], HD) for v in range(self.n)]
        self.o = [O.FrameHashes(pairs(v, 0), pairs(v, 1) if self.endings else [], HD, "") for v in range(self.n)]

    def comparators(self, min_s, threshold=10, padding=0.0):
        c = capi.Comparator(self.paths, include_endings=self.endings, hash_match_threshold=threshold, min_opening_duration=min_s,
                            min_ending_duration=min_s, time_padding=padding)
        o = O.Comparator(include_endings=self.endings, hash_match_threshold=threshold, min_opening_duration=min_s * NS,
                         min_ending_duration=min_s * NS, time_padding=O.duration_from_secs_f32(padding))
        return c, o

    def oracle_per_group(self, ocmp, labels, threads=8):
        want = [None] * self.n
        for m in members_of(labels):
            for v, r in zip(m, O.run_with_frame_hashes(ocmp, [self.o[v] for v in m], threads=threads)):
                want[v] = r
        return _as(want)


def both_forms(monkeypatch, call):
    out = []
    for form in FORMS:
        monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", form)
        out.append(call())
    return out


def test_no_match_crosses_a_group_and_ungrouped_one_does(monkeypatch):
    """12 videos in 4 interleaved groups (5, 4, 2 and one alone).  The groups of five and of four share an exact segment of
    ~30 s each; video 0 (group A) and video 1 (group B) also share an exact segment of ~60 s -- which the ungrouped call
    prefers for both (duration weighs 0.7), and the grouped call must never see."""
    A, B, C2, ALONE = 0xFFFFFFFF, 0, 77, 5
    labels = [A, B, A, C2, B, A, ALONE, B, A, C2, B, A]
    rng = np.random.default_rng(11)
    rows = random_rows(rng, [600 + 7 * v for v in range(12)])
    for label, at in ((A, 20), (B, 60), (C2, 100)):
        seg = rng.integers(0, 2 ** 32, 122, dtype=np.uint64).astype(np.uint32)
        for k, v in enumerate(members_of(labels)[[A, B, C2].index(label)]):
            rows[v][0][at + 9 * k: at + 9 * k + len(seg)] = seg
    cross = rng.integers(0, 2 ** 32, 244, dtype=np.uint64).astype(np.uint32)
    rows[0][0][300:300 + 244] = cross
    rows[1][0][330:330 + 244] = cross
    videos = Videos(rows, even_timestamps(rows))
    cmp, ocmp = videos.comparators(min_s=20)
    want = videos.oracle_per_group(ocmp, labels)
    for got in both_forms(monkeypatch, lambda: _as(cmp.run_with_frame_hashes(videos.c, groups=labels))):
        assert got == want
        assert got[6] is None and all(got[v] is not None and got[v][0] is not None for v in range(12) if v != 6)
    ungrouped = _as(cmp.run_with_frame_hashes(videos.c))
    assert ungrouped == _as(O.run_with_frame_hashes(ocmp, videos.o, threads=8))
    for v in (0, 1):                                                     # the case has teeth: all pairs would answer otherwise
        assert ungrouped[v][0] != want[v][0] and ungrouped[v][0][1] - ungrouped[v][0][0] > 50 * NS > want[v][0][1] - want[v][0][0]
    assert [ungrouped[v] for v in range(2, 12) if v != 6] == [want[v] for v in range(2, 12) if v != 6]


def test_a_group_of_258_crosses_the_256_slot_stage(monkeypatch):
    """best_match_kernel takes a video's pair slots 256 at a time: one group of 258 (257 slots a video) interleaved with a
    group of 5, rows of 100-130 hashes of unequal lengths."""
    labels = []
    for v in range(258):
        labels.append(9)
        if v % 60 == 7:
            labels.append(0xFFFFFFFF)
    rng = np.random.default_rng(12)
    rows = random_rows(rng, [100 + int(x) for x in rng.integers(0, 31, len(labels))])
    seg9, seg5 = (rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32) for k in (40, 52))
    for v, label in enumerate(labels):
        seg = seg9 if label == 9 else seg5
        at = 3 + (v * 7) % 40
        flips = (np.uint32(1) << rng.integers(0, 32, len(seg)).astype(np.uint32)) * (rng.random(len(seg)) < 0.2)
        rows[v][0][at:at + len(seg)] = seg ^ (flips.astype(np.uint32) if v % 3 else np.uint32(0))   # a third of them exact copies
    videos = Videos(rows, even_timestamps(rows))
    cmp, ocmp = videos.comparators(min_s=5)
    want = videos.oracle_per_group(ocmp, labels, threads=16)
    assert sum(1 for r in want if r is not None and r[0] is not None) >= 250
    for got in both_forms(monkeypatch, lambda: _as(cmp.run_with_frame_hashes(videos.c, groups=labels))):
        assert got == want


def _constant_stretch_library(rng, kept, stretch, small=300):
    """Two groups: videos 0, 2 (and 4, short rows) are one; 1, 3 the other.  Videos 0 and 2 hold one hash `stretch` times."""
    labels = [3, 8, 3, 8, 3]
    rows = random_rows(rng, [kept, small, kept, small, small])
    for k, v in enumerate((0, 2)):
        rows[v][0][30 + 7 * k: 30 + 7 * k + stretch] = np.uint32(0x0F1E2D3C)
    seg = rng.integers(0, 2 ** 32, 90, dtype=np.uint64).astype(np.uint32)
    for v in range(5):
        rows[v][0][small - 100: small - 10] = seg                        # an ordinary segment everybody shares, across groups too
    return labels, Videos(rows, even_timestamps(rows))


def test_buckets_beyond_a_lane_and_beyond_a_workgroup(monkeypatch):
    """A pair of constant stretches of 40 hashes inside one group: ~39 runs of 21 and more in one bucket, past the 24 one lane
    orders -- pair_entries_large_kernel<GroupedPairs>, no fallback.  Stretches of 4 210: ~8 250 runs, past what that kernel
    holds in LDS -- the host form from the downloaded list, counted once, and only there."""
    cases = {}
    for name, kept, stretch in (("lane", 300, 40), ("workgroup", 4500, 4210)):
        labels, videos = _constant_stretch_library(np.random.default_rng(13), kept, stretch)
        cmp, ocmp = videos.comparators(min_s=5)
        cases[name] = (labels, videos, cmp, videos.oracle_per_group(ocmp, labels))
    for name, fallbacks in (("lane", 0), ("workgroup", 1)):
        labels, videos, cmp, want = cases[name]
        for form in FORMS:
            monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", form)
            capi.epilogue_host_fallbacks(reset=True)
            got = _as(cmp.run_with_frame_hashes(videos.c, groups=labels))
            assert capi.epilogue_host_fallbacks(reset=True) == (fallbacks if form == "1" else 0), (name, form)
            assert got == want, (name, form)
            assert all(r is not None and r[0] is not None for r in got)


def test_endings_unequal_lengths_and_timestamps_nobody_shares(monkeypatch):
    """Both regions, rows of unequal lengths, every video its own timestamp step and origin; segments shared inside the groups
    and, longer, across them (which must not count)."""
    labels = [1, 2, 1, 3, 2, 1, 2, 3, 1]
    rng = np.random.default_rng(14)
    rows = random_rows(rng, [380 + 17 * v for v in range(len(labels))], regions=2)
    for m in members_of(labels):
        for r in range(2):
            seg = rng.integers(0, 2 ** 32, 110 + 12 * r, dtype=np.uint64).astype(np.uint32)
            for k, v in enumerate(m):
                flips = (np.uint32(1) << rng.integers(0, 32, len(seg)).astype(np.uint32)) * (rng.random(len(seg)) < 0.3)
                rows[v][r][10 + 11 * k + 5 * r: 10 + 11 * k + 5 * r + len(seg)] = seg ^ flips.astype(np.uint32)
    for r in range(2):
        cross = rng.integers(0, 2 ** 32, 200, dtype=np.uint64).astype(np.uint32)
        rows[0][r][170:370] = cross
        rows[1][r][175:375] = cross
        rows[3][r][160:360] = cross
    ts = [[[2_000_000_000 + 1_000_003 * v + 5_000 * NS * r + i * (STEP + 1_000 * v) for i in range(len(row))]
           for r, row in enumerate(video)] for v, video in enumerate(rows)]
    videos = Videos(rows, ts)
    cmp, ocmp = videos.comparators(min_s=15, padding=0.5)
    want = videos.oracle_per_group(ocmp, labels)
    assert all(r is not None and r[0] is not None and r[1] is not None for r in want)
    for got in both_forms(monkeypatch, lambda: _as(cmp.run_with_frame_hashes(videos.c, groups=labels))):
        assert got == want
    assert _as(cmp.run_with_frame_hashes(videos.c))[0] != want[0]       # (all pairs: the cross segment wins)


def test_a_failing_video_fails_the_call_at_the_lowest_position(monkeypatch, capfd):
    """Padding of 40 s: a video whose match ends before 40 s fails (the reference panics on the subtraction).  Videos 3 and 6
    (different groups) are such; the call fails in both forms after printing videos 0-2 and the header of video 3."""
    labels = [4, 5, 4, 5, 4, 5, 4, 6]
    rng = np.random.default_rng(15)
    rows = random_rows(rng, [560] * len(labels))
    for m in members_of(labels)[:2]:
        seg = rng.integers(0, 2 ** 32, 122, dtype=np.uint64).astype(np.uint32)
        for k, v in enumerate(m):
            at = 2 if v in (3, 6) else 300 + 9 * k                       # ends at 2.6 + 124 * 0.246 s = 33 s, or beyond 100 s
            rows[v][0][at:at + len(seg)] = seg
    videos = Videos(rows, even_timestamps(rows))
    cmp, _ = videos.comparators(min_s=20, padding=40.0)
    texts = []
    for form in FORMS:
        monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", form)
        capfd.readouterr()
        with pytest.raises(capi.NeedleError, match="overflow when subtracting durations"):
            cmp.run_with_frame_hashes(videos.c, display=True, groups=labels)
        texts.append(capfd.readouterr().out)
    assert texts[0] == texts[1]
    assert texts[0].count("* Opening - ") == 3 and texts[0].endswith("\nv3.mkv\n\n") and "v4.mkv" not in texts[0]
    fine, ocmp = videos.comparators(min_s=20, padding=1.0)              # the same library fails nobody at 1 s
    assert _as(fine.run_with_frame_hashes(videos.c, groups=labels)) == videos.oracle_per_group(ocmp, labels)


def test_one_group_is_the_ungrouped_call_byte_for_byte(monkeypatch, capfd, tmp_path):
    """Results, printed lines and skip files; and groups=None is the ungrouped call."""
    n = 7
    rng = np.random.default_rng(16)
    rows = random_rows(rng, [420 + 13 * (v % 3) for v in range(n)], regions=2)
    for r in range(2):
        seg = rng.integers(0, 2 ** 32, 115, dtype=np.uint64).astype(np.uint32)
        for v in range(n - 1):                                           # the last video shares nothing: "No opening or ending found."
            rows[v][r][12 + 17 * v: 12 + 17 * v + len(seg)] = seg
    paths = [str(tmp_path / f"ep{v}.mkv") for v in range(n)]
    for v, p in enumerate(paths):
        with open(p, "wb") as f:
            f.write(rng.integers(0, 256, 8192 + v, dtype=np.uint8).tobytes())       # (the skip file names the md5 of the first 8 KiB)
    videos = Videos(rows, even_timestamps(rows), paths)
    cmp, ocmp = videos.comparators(min_s=15, padding=0.5)
    skip_of = lambda p: p[:-4] + ".needle.skip.json"

    def call(groups):
        for p in paths:
            if os.path.exists(skip_of(p)):
                os.unlink(skip_of(p))
        capfd.readouterr()
        res = _as(cmp.run_with_frame_hashes(videos.c, display=True, write_skip_files=True, groups=groups))
        return res, capfd.readouterr().out, {p: open(skip_of(p), "rb").read() for p in paths if os.path.exists(skip_of(p))}

    for form in FORMS:
        monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", form)
        plain = call(None)
        assert plain[0] == _as(O.run_with_frame_hashes(ocmp, videos.o, threads=8))
        assert len(plain[2]) == n - 1 and plain[1].count('* Opening - "') == n - 1 and "No opening or ending found." in plain[1]
        for label in (0, 0xFFFFFFFF, 12345):
            assert call([label] * n) == plain, (form, label)


def test_launches_do_not_depend_on_the_number_of_groups(monkeypatch):
    """The same 24 videos as one group and as eight: the same number of scan and of epilogue launches."""
    n = 24
    rng = np.random.default_rng(17)
    rows = random_rows(rng, [400] * n)
    seg = rng.integers(0, 2 ** 32, 100, dtype=np.uint64).astype(np.uint32)
    for v in range(n):
        rows[v][0][20 + 3 * v: 120 + 3 * v] = seg
    videos = Videos(rows, even_timestamps(rows))
    cmp, ocmp = videos.comparators(min_s=10)
    names = ("hamming_runs", "hamming_runs_unstaged", "simhash_runs", "epilogue_buckets", "epilogue_entries", "epilogue_best_match")
    monkeypatch.setenv("NEEDLE_HIP_DEVICE_EPILOGUE", "1")
    counts = {}
    for groups in ([1] * n, [v % 8 for v in range(n)]):
        cmp.run_with_frame_hashes(videos.c, groups=groups)                # (tables and workspaces of this shape are up)
        capi.set_kernel_timing("all,sum")
        try:
            got = _as(cmp.run_with_frame_hashes(videos.c, groups=groups))
            counts[len(set(groups))] = {k: capi.kernel_launches(k) for k in names}
        finally:
            capi.set_kernel_timing(None)
        assert got == videos.oracle_per_group(ocmp, groups)
    print(counts)
    assert counts[1] == counts[8]
    assert counts[8]["epilogue_best_match"] == 1 and counts[8]["epilogue_entries"] == 1 and counts[8]["epilogue_buckets"] == 1
    assert counts[8]["hamming_runs"] + counts[8]["hamming_runs_unstaged"] >= 1


def test_cli_group_by_dir_is_needle_search_per_directory(tmp_path):
    """Three directories of three short WAVs under one root: per file, `needle search --group-by-dir <root>` (a directory
    stands for its sub-directories there) prints what `needle search <its directory>` prints, and writes the same skip file."""
    exe = os.path.join(os.path.dirname(os.path.dirname(capi.LIB_PATH)), "bin", "needle")
    assert os.path.exists(exe), "build() builds the command line"
    dirs = []
    for d in range(3):
        eps = synth.make_library(3, 80.0 + 6.0 * d, 18.0 + 2.0 * d, seed_base=synth.EPISODE_SEED + 1000 * d)
        os.makedirs(tmp_path / f"show{d}")
        dirs.append([])
        for k, e in enumerate(eps):
            p = str(tmp_path / f"show{d}" / f"s01e0{k}.wav")
            synth.write_wav(p, e.pcm, channels=1)
            dirs[-1].append(p)
    r = subprocess.run([exe, "analyze", *[str(tmp_path / f"show{d}") for d in range(3)]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    flags = ["--min-opening-duration", "10", "--write-skip-files"]
    skip_of = lambda p: p[:-4] + ".needle.skip.json"
    per_dir_text, per_dir_skips = "", {}
    for d in range(3):
        r = subprocess.run([exe, "search", str(tmp_path / f"show{d}"), *flags], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        per_dir_text += r.stdout
        for p in dirs[d]:
            per_dir_skips[p] = open(skip_of(p), "rb").read()
            os.unlink(skip_of(p))
    assert per_dir_text.count('* Opening - "') == 9
    r = subprocess.run([exe, "search", "--group-by-dir", str(tmp_path), *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == per_dir_text                                      # (sorted paths: directory after directory)
    assert {p: open(skip_of(p), "rb").read() for ps in dirs for p in ps} == per_dir_skips
    h = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert "--group-by-dir" in h.stdout
