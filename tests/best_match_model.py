"""A small NumPy model of find_best_match (comparator.rs:405-515) that also says WHY: the winner's pair, its index in the
candidate list, how many candidates support it and from how many partners -- the reference of needle_hip.h's
NeedleHipMatchEvidence in tests/test_evidence_cpu.py and tests/test_gpu_index_evidence.py.

Precondition: EVERY (pair, region) bucket holds AT MOST ONE run (assert_one_run_per_bucket).  Then no heap order is involved:
the candidate list of video v is one entry per partner q in the reference's pair order -- (q, v) for q < v, where v is the
destination, then (v, q) for q > v, where v is the source (:534-545) -- openings before endings within a pair (:414-431).
Links, count and score are np.float32 with a separate multiply and add (:469); a candidate nobody links to, itself included
(`count == 0`: only at threshold 0), is skipped; argmin breaks ties to the lower index (:473-475).

Also here: the oracle's run list of a library in the form the host epilogue takes (oracle_runs), and the planted library both
test files use (planted_library)."""
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from needle_amd import capi
from oracle import oracle as O

NS = O.NS
HD = O.duration_from_secs_f32(0.3)
TS0, STEP, ENDING_SHIFT = 2_600_000_000, 246_000_000, 7_000 * NS


def min_len_for(min_s: int, step: int = STEP) -> int:
    """Comparator::min_run_length over evenly spaced timestamps: the fewest steps that span the minimum duration."""
    return -(-min_s * NS // step)


def oracle_runs(rows, threshold: int, min_len: int, threads: int = 4) -> np.ndarray:
    """The oracle's table-free scan of every pair, region by region, as capi.RUN_DTYPE: problem = pair (i-major) * regions
    + region, the simhashes of both sides over the run's len + 1 hashes (:149-153,226-229)."""
    n, regions = len(rows), len(rows[0])
    out = []
    for r in range(regions):
        seqs = [np.ascontiguousarray(rows[v][r], dtype=np.uint32) for v in range(n)]
        total, runs = O.diagonal_runs_all_pairs(seqs, threshold, min_len, threads=threads, capacity=2 * n * n + 1024)
        if total > len(runs):
            total, runs = O.diagonal_runs_all_pairs(seqs, threshold, min_len, threads=threads, capacity=total)
        assert total == len(runs)
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
        for p, i_end, j_end, ln in runs.tolist():
            i, j = pairs[p]
            out.append((p * regions + r, i_end, j_end, ln, O.simhash32(seqs[i][i_end - ln:i_end + 1]),
                        O.simhash32(seqs[j][j_end - ln:j_end + 1])))
    arr = np.zeros(len(out), dtype=capi.RUN_DTYPE)
    for k, name in enumerate(capi.RUN_DTYPE.names):
        arr[name] = [x[k] for x in out]
    return arr


def assert_one_run_per_bucket(runs: np.ndarray) -> None:
    """The model's precondition, on a run list."""
    if len(runs):
        crowd = np.bincount(runs["problem"].astype(np.int64)).max()
        assert crowd == 1, f"a (pair, region) bucket holds {crowd} runs: the model does not cover this library"


@dataclass
class ModelEvidence:                                     # capi.MatchEvidence, field for field
    partner: int
    is_source: bool
    candidate: int
    candidates: int
    support: int
    partners: int
    score: np.float32
    match_hash: int
    partner_hash: int
    interval: Tuple[int, int]
    partner_interval: Tuple[int, int]


def as_secs_f32(ns: int) -> np.float32:                  # Duration::as_secs_f32
    return np.float32(ns // NS) + np.float32(ns % NS) / np.float32(NS)


def _popcount(x: np.ndarray) -> np.ndarray:
    return np.unpackbits(x.astype(">u4").view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1)


def evidence_model(ts, runs: np.ndarray, threshold: int, min_ns: Tuple[int, int], include_endings: bool, padding: int = 0,
                   hash_duration: int = HD):
    """ts[v][r]: the timestamps of video v's row r.  Returns (results, evidence): per video None where it has no candidate
    at all, else ((opening, ending) intervals or None, (ModelEvidence or None) x 2)."""
    assert_one_run_per_bucket(runs)
    n, regions = len(ts), len(ts[0])
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    bucket: Dict[int, dict] = {}
    for run in runs:
        p, r = divmod(int(run["problem"]), regions)
        i, j = pairs[p]
        i_end, j_end, ln = int(run["src_end"]), int(run["dst_end"]), int(run["len"])
        src = (int(ts[i][r][i_end - ln]), int(ts[i][r][i_end]))       # one BEFORE the first matched cell (:206-207)
        dst = (int(ts[j][r][j_end - ln]), int(ts[j][r][j_end]))
        if src[1] - src[0] < min_ns[r] or dst[1] - dst[0] < min_ns[r]:   # :212-223
            continue
        bucket[int(run["problem"])] = dict(src=src, dst=dst, src_hash=int(run["src_match_hash"]), dst_hash=int(run["dst_match_hash"]))
    bound = threshold + threshold // 2                   # :441
    # per video (partner, is_source, region, mine, theirs, my hash, their hash) in (partner, region) order: partners below v
    # are its sources, those above its destinations, so this is the reference's pair order
    lists = [[] for _ in range(n)]
    for problem in sorted(bucket):
        e = bucket[problem]
        p, r = divmod(problem, regions)
        i, j = pairs[p]
        lists[i].append((j, True, r, e["src"], e["dst"], e["src_hash"], e["dst_hash"]))
        lists[j].append((i, False, r, e["dst"], e["src"], e["dst_hash"], e["src_hash"]))
    results, evidence = [], []
    for v in range(n):
        cand = sorted(lists[v], key=lambda c: (c[0], c[2]))
        if not cand:
            results.append(None)
            evidence.append((None, None))
            continue
        hashes = np.array([c[5] for c in cand], dtype=np.uint32)
        near = np.array([_popcount(hashes ^ h) < bound for h in hashes])            # [k][b], symmetric
        links = near.sum(axis=1)
        res, ev = [None, None], [None, None]
        for which in range(2 if include_endings else 1):
            best: Optional[int] = None
            best_key = None
            for k, c in enumerate(cand):
                if c[2] != which or links[k] == 0:       # `count == 0`: nobody within the bound, not even itself (t = 0)
                    continue
                weighted = np.float32(links[k]) * np.float32(0.3) + as_secs_f32(c[3][1] - c[3][0]) * np.float32(0.7)
                key = -weighted
                if best is None or key < best_key:       # ascending (key, index), first
                    best, best_key = k, key
            if best is None:
                continue
            c = cand[best]
            res[which] = (c[3][0] + padding, c[3][1] - padding - hash_duration)     # :479, :481
            ev[which] = ModelEvidence(c[0], c[1], best, len(cand), int(links[best]),
                                      len({cand[b][0] for b in range(len(cand)) if near[best][b]}), np.float32(-best_key), c[5], c[6],
                                      c[3], c[4])
        results.append(tuple(res))
        evidence.append(tuple(ev))
    return results, evidence


def same_evidence(got, want) -> bool:
    """capi.MatchEvidence against ModelEvidence (or another capi.MatchEvidence): every field, the score bit for bit."""
    if got is None or want is None:
        return got is None and want is None
    fields = ("partner", "is_source", "candidate", "candidates", "support", "partners", "match_hash", "partner_hash", "interval",
              "partner_interval")
    return all(getattr(got, f) == getattr(want, f) for f in fields) and \
        np.float32(got.score).tobytes() == np.float32(want.score).tobytes()


def planted_library(seed: int, endings: bool, n: int = 6, kept: int = 600):
    """rows[v][r]: n videos of `kept` random hashes with one opening (110 hashes) shared by videos 0-3, a second, longer one
    (150) shared by videos 3-5 and, with endings, video 5's ending (120) planted in videos 1 and 4; here and there a flipped
    bit (threshold 10).  Video 3 holds both openings."""
    rng = np.random.default_rng(seed)
    new = lambda k: rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
    rows = [[new(kept) for _ in range(2 if endings else 1)] for _ in range(n)]

    def plant(seg, places):
        for v, r, at in places:
            flips = (np.uint32(1) << rng.integers(0, 32, len(seg)).astype(np.uint32)) * (rng.random(len(seg)) < 0.3)
            rows[v][r][at:at + len(seg)] = seg ^ flips.astype(np.uint32)

    plant(new(110), [(0, 0, 20), (1, 0, 33), (2, 0, 46), (3, 0, 7)])
    plant(new(150), [(3, 0, 300), (4, 0, 250), (5, 0, 410)])
    if endings:
        plant(new(120), [(5, 1, 400), (1, 1, 90), (4, 1, 231)])
    return rows


def timestamps(rows):
    """What Corpus.add_rows (tests/test_gpu_index.py) gives these rows."""
    return [[[TS0 + (ENDING_SHIFT if r else 0) + i * STEP for i in range(len(row))] for r, row in enumerate(video)] for video in rows]
