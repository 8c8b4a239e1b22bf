"""Libraries whose candidate lists are chosen hash by hash, for the link counts of find_best_match (comparator.rs:434-454):
links[k] = #{b : popcount(h_k ^ h_b) < bound}, bound = t + t / 2.  Plain NumPy, no device: tests/test_link_tables_cpu.py
proves the tables against the oracle, tests/test_gpu_link_counts.py runs them through best_match_kernel.

A hub and its spokes.  A candidate's hash is the simhash of its run's len + 1 hashes, rows[i_end - len : i_end + 1]: the row
before the first matched cell through the last cell.  The simhash is a bitwise strict majority, so XORing M ^ H into all of an
ODD number of random rows whose simhash is M makes it H and leaves the rows random-looking.  A hub video holds one such
segment per target, each copied bit for bit into a spoke video and fenced there by the hub's neighbouring rows XOR a mask of
t + 1 bits: the run is exactly the planted cells.  All segments are equally long and timestamps evenly spaced, so all of the
hub's candidates have the same duration: the links alone decide the hub's winner, ties go to the lower index.  The hub comes
before its spokes, so it is the source of every pair and its candidate k is spoke k's segment, in spoke order; with endings
the segments alternate between the two regions (both regions' candidates share one list and link across regions)."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

GAP = 2                                 # random rows between two segments, beyond the fenced rows


def popcount(x) -> np.ndarray:
    return np.bitwise_count(np.asarray(x, dtype=np.uint32)).astype(np.int64)


def simhash(rows: np.ndarray) -> int:
    """ora_simhash32: bit b is set where more than half of the rows have it (a tie clears it)."""
    bits = (np.asarray(rows, dtype=np.uint32)[:, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    ones = bits.sum(axis=0, dtype=np.int64)
    return int(((2 * ones > len(rows)).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum())


def _random(rng, k: int) -> np.ndarray:
    return rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)


def mask_of(rng, weight: int) -> int:
    """A u32 with exactly `weight` set bits."""
    return int(sum(1 << int(b) for b in rng.permutation(32)[:weight]))


def cells_for(min_len: int) -> int:
    """Cells of a planted segment: at least min_len, and even, so that its len + 1 rows have no tie."""
    return min_len + (min_len & 1)


def _layout(sizes: Sequence[int], min_len: int, endings: bool, per_spoke=1):
    """Where everything goes: (regions, cells, stride, at, spokes).  at[h][k]: the first cell of hub h's segment k in its region
    k % regions; spokes: per spoke video, the (hub, segment) it holds, in the order they are planted in it."""
    regions, cells = (2 if endings else 1), cells_for(min_len)
    stride = cells + 2 + GAP
    at = [[2 + (k // regions) * stride for k in range(c)] for c in sizes]
    spokes = []
    for h, c in enumerate(sizes):
        shares = [per_spoke] * (c // per_spoke) if isinstance(per_spoke, int) else [int(s) for s in per_spoke]
        assert sum(shares) == c and min(shares) >= 1, (shares, c)
        k0 = 0
        for s in shares:
            spokes.append([(h, k) for k in reversed(range(k0, k0 + s))])
            k0 += s
    return regions, cells, stride, at, spokes


def hubs_library(tables: Sequence[Sequence[int]], t: int, min_len: int, endings: bool, seed: int, per_spoke=1):
    """rows[v][r] of a library of len(tables) hubs (the first videos) and then every hub's spokes in turn.  tables[h]: hub h's
    targets.  per_spoke: an int, or one count per spoke (they sum to the targets), the same for every hub; a spoke of s > 1
    holds s consecutive targets, planted in reverse order, so that each is a run on a diagonal of its own (with endings they
    alternate between the regions: a spoke of two holds one run per bucket)."""
    rng = np.random.default_rng(seed)
    regions, cells, stride, at, spokes = _layout([len(tb) for tb in tables], min_len, endings, per_spoke)
    hubs = []
    for h, targets in enumerate(tables):
        hub = [_random(rng, 1 + max(1, -(-len(targets) // regions)) * stride) for _ in range(regions)]
        for k, target in enumerate(targets):     # the hub's segment k: rows at - 1 (before the first cell) .. at + cells - 1
            seg = hub[k % regions][at[h][k] - 1:at[h][k] + cells]
            seg ^= np.uint32(simhash(seg) ^ int(target))
        hubs.append(hub)
    rows, planted = list(hubs), []               # planted: (hub video, spoke video, region, hub row, spoke row, target)
    for held in spokes:
        spoke = []
        for r in range(regions):
            here = [(h, k) for h, k in held if k % regions == r]
            row = _random(rng, 1 + max(1, len(here)) * stride)
            for slot, (h, k) in enumerate(here):
                a, b = at[h][k], 2 + slot * stride
                row[b:b + cells] = hubs[h][r][a:a + cells]
                row[b - 1] = hubs[h][r][a - 1] ^ np.uint32(mask_of(rng, t + 1))
                row[b + cells] = hubs[h][r][a + cells] ^ np.uint32(mask_of(rng, t + 1))
                planted.append((h, len(rows), r, a, b, int(tables[h][k])))
            spoke.append(row)
        rows.append(spoke)
    for h, q, r, a, b, target in planted:        # what was planted is what was meant
        assert not (rows[h][r][a:a + cells] ^ rows[q][r][b:b + cells]).any(), "a planted cell is not at distance 0"
        assert popcount(rows[h][r][a - 1] ^ rows[q][r][b - 1]) == t + 1 == popcount(rows[h][r][a + cells] ^ rows[q][r][b + cells])
        assert simhash(rows[h][r][a - 1:a + cells]) == target, "a segment's simhash is not its target"
    return rows


def hub_library(targets: Sequence[int], t: int, min_len: int, endings: bool, seed: int, per_spoke=1):
    """One hub (video 0) and its spokes: see hubs_library."""
    return hubs_library([targets], t, min_len, endings, seed, per_spoke)


def planted_runs(tables, min_len: int, endings: bool, per_spoke=1):
    """What oracle_runs must find in hubs_library's rows and nothing else: a sorted list of (problem, src_end, dst_end, len),
    problem = pair (i-major over all videos) * regions + region."""
    regions, cells, stride, at, spokes = _layout([len(tb) for tb in tables], min_len, endings, per_spoke)
    n = len(tables) + len(spokes)
    out = []
    for q, held in enumerate(spokes, start=len(tables)):
        for r in range(regions):
            here = [(h, k) for h, k in held if k % regions == r]
            for slot, (h, k) in enumerate(here):
                pair = h * n - h * (h + 1) // 2 + (q - h - 1)
                out.append((pair * regions + r, at[h][k] + cells - 1, 2 + slot * stride + cells - 1, cells))
    return sorted(out)


def _distinct_near(rng, centre: int, weights: Sequence[int], count: int, taken: set) -> List[int]:
    """`count` values, different from each other and from `taken`, each centre ^ a mask whose weight is drawn from `weights`."""
    out = []
    while len(out) < count:
        x = centre ^ mask_of(rng, int(rng.choice(weights)))
        if x not in taken:
            taken.add(x)
            out.append(x)
    return out


def edge_targets(bound: int, seed: int) -> np.ndarray:
    """Sixteen targets at the bound's edge, in shuffled order: two centres A and B = ~A, four satellites of A at distance
    exactly bound - 1 and two at bound, three satellites of B at bound - 1 and five at bound."""
    assert 1 <= bound <= 32
    rng = np.random.default_rng(seed)
    a = int(_random(rng, 1)[0])
    b = a ^ 0xFFFFFFFF
    out = [a, b]
    for centre, inside, outside in ((a, 4, 2), (b, 3, 5)):
        out += [centre ^ mask_of(rng, bound - 1) for _ in range(inside)] + [centre ^ mask_of(rng, bound) for _ in range(outside)]
    out = np.array(out, dtype=np.uint32)
    assert popcount(out[2:8] ^ np.uint32(a)).tolist() == [bound - 1] * 4 + [bound] * 2
    assert popcount(out[8:] ^ np.uint32(b)).tolist() == [bound - 1] * 3 + [bound] * 5
    return out[rng.permutation(16)]


def seam_positions(c: int) -> List[int]:
    """Where a block, a tile half or a stage of the matrix path begins or ends, below c: the sixteen-row seam 15 | 16, the
    blocks' 31 | 32 and 63 | 64, the stages' 511 | 512, 1023 | 1024 and 1535 | 1536, the last block's first row and the last two
    candidates."""
    last_block = (c - 1) // 32 * 32
    want = {0, 15, 16, 31, 32, 63, 64, 511, 512, 1023, 1024, 1535, 1536, last_block, c - 2, c - 1}
    return sorted(p for p in want if 0 <= p < c)


def cluster_targets(c: int, bound: int, seed: int) -> np.ndarray:
    """c pairwise different targets, the A / B table scaled up.  A clique -- A and values within (bound - 1) / 2 bits of it,
    which all link to each other -- holds every seam position (seam_positions) and three of every four others; the rest are
    at bound .. bound + 3 bits from A (around B = ~A), which never link to A.  The winner is of the clique, and its support has
    members on both sides of every seam, in every block and in every stage."""
    assert bound >= 3
    rng = np.random.default_rng(seed)
    a = int(_random(rng, 1)[0])
    seams = set(seam_positions(c))
    in_clique = [k in seams or k % 4 != 3 for k in range(c)]
    taken = {a}
    near = _distinct_near(rng, a, list(range(1, (bound - 1) // 2 + 1)), sum(in_clique) - 1, taken)
    far = _distinct_near(rng, a, list(range(bound, min(32, bound + 3) + 1)), c - sum(in_clique), taken)
    near.insert(int(rng.integers(0, len(near) + 1)), a)
    out = np.array([near.pop() if inside else far.pop() for inside in in_clique], dtype=np.uint32)
    assert len(set(out.tolist())) == c
    return out


def home_slot(h) -> np.ndarray:
    """The dedup table's home slot of a hash, mirrored from best_match_kernel's slot_of (csrc/epilogue_kernels.h):
    (hash * 0x9E3779B1 mod 2^32) >> 21, one of 2048."""
    return ((np.asarray(h, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(21)


SLOTS = 2048                            # best_match_kernel's kSlots


def palette_targets(c: int, distinct: int, seed: int, collide: bool = False) -> np.ndarray:
    """c targets drawn from `distinct` random values, every value used at least once.  collide: four of the values have home
    slot 2047 and three have 2046 -- seven keys for two slots, so whatever the order of insertion, linear probing takes at
    least five of them past the table's end to slots 0 .. 4."""
    assert 1 <= distinct <= c
    rng = np.random.default_rng(seed)
    values: List[int] = []
    taken: set = set()
    if collide:
        assert distinct >= 7
        for slot, count in ((SLOTS - 1, 4), (SLOTS - 2, 3)):
            have = 0
            while have < count:
                draw = _random(rng, 1 << 16)
                for x in draw[home_slot(draw) == slot].tolist():
                    if x not in taken and have < count:
                        taken.add(x)
                        values.append(x)
                        have += 1
    while len(values) < distinct:
        x = int(_random(rng, 1)[0])
        if x not in taken:
            taken.add(x)
            values.append(x)
    values = np.array(values, dtype=np.uint32)
    picks = np.concatenate([np.arange(distinct), rng.integers(0, distinct, c - distinct)])
    out = values[picks[rng.permutation(c)]]
    assert len(set(out.tolist())) == distinct
    if collide:
        slots = home_slot(np.unique(out))
        assert (slots == SLOTS - 1).sum() >= 4 and (slots == SLOTS - 2).sum() >= 3
    return out


def table_slots(hashes, wrap: bool = True) -> dict:
    """The dedup table as best_match_kernel fills it, one insertion at a time (under linear probing the set of occupied slots
    does not depend on the order): {hash: slot}.  wrap=False: the probe sequence WITHOUT its wrap, sl + 1 in place of
    (sl + 1) & (kSlots - 1) -- slots beyond the table."""
    at, used = {}, set()
    for h in np.asarray(hashes, dtype=np.uint32).tolist():
        if h in at:
            continue
        sl = int(home_slot(h))
        while sl in used:
            sl = (sl + 1) % SLOTS if wrap else sl + 1
        used.add(sl)
        at[h] = sl
    return at


def links(hashes, bound: int) -> np.ndarray:
    """links[k] = #{b : popcount(h_k ^ h_b) < bound}, k itself included (comparator.rs:434-454): the O(c^2) count."""
    h = np.asarray(hashes, dtype=np.uint32)
    out = np.zeros(len(h), dtype=np.int64)
    for lo in range(0, len(h), 256):
        out[lo:lo + 256] = (popcount(h[lo:lo + 256, None] ^ h[None, :]) < bound).sum(axis=1)
    return out


def winner(hashes, is_opening, bound: int) -> Tuple[Optional[Tuple[int, int]], Optional[Tuple[int, int]]]:
    """(index, support) of the opening's and of the ending's winner among candidates of EQUAL duration: the most links of its
    region, the lower index on a tie; a candidate without links is skipped (ora_needle.c:720, comparator.rs `count == 0`), a
    region without a linked candidate has None.  is_opening: per candidate, or one bool for all."""
    count = links(hashes, bound)
    opening = np.broadcast_to(np.asarray(is_opening, dtype=bool), count.shape)
    out = []
    for which in (True, False):
        idx = np.flatnonzero((opening == which) & (count > 0))
        if len(idx) == 0:
            out.append(None)
            continue
        # (the score -(links * 0.3 + secs * 0.7) in f32: one link more is 0.3, far above an ulp at any count a test reaches)
        best = idx[np.argmax(count[idx])]                # argmax: the first of the largest
        out.append((int(best), int(count[best])))
    return tuple(out)


# ---- the cases both test modules run ------------------------------------------------------------------------------------------
# bound -> edge_targets seed: the first that proves itself at every rotation (tests/test_link_tables_cpu.py)
EDGE_SEEDS = {1: 1, 3: 1, 15: 1, 16: 1, 18: 2, 21: 16}
MIN_S = 5                                                # seconds: min_len 21 at 246 ms a hash, segments of 22 cells


class Case:
    """A hub library: tables[h] are hub h's targets, in candidate order."""

    def __init__(self, name, t, tables, endings=False, per_spoke=1, seed=0, one_run_per_bucket=True):
        self.name, self.t, self.endings, self.per_spoke, self.seed = name, t, endings, per_spoke, seed
        self.tables = [np.asarray(tb, dtype=np.uint32) for tb in tables]
        self.bound = t + t // 2
        self.min_s = MIN_S
        self.min_len = -(-MIN_S * 1_000_000_000 // 246_000_000)
        self.one_run_per_bucket = one_run_per_bucket
        self._rows = None

    def rows(self):
        if self._rows is None:
            self._rows = hubs_library(self.tables, self.t, self.min_len, self.endings, self.seed, self.per_spoke)
        return self._rows

    def planted(self):
        return planted_runs(self.tables, self.min_len, self.endings, self.per_spoke)

    def spoke_of(self, h, k):
        """The video that holds hub h's segment k."""
        spokes = _layout([len(tb) for tb in self.tables], self.min_len, self.endings, self.per_spoke)[4]
        return len(self.tables) + next(q for q, held in enumerate(spokes) if (h, k) in held)

    def is_opening(self, h):
        return np.arange(len(self.tables[h])) % (2 if self.endings else 1) == 0

    def winners(self, h, bound=None):
        return winner(self.tables[h], self.is_opening(h), self.bound if bound is None else bound)

    def __repr__(self):
        return self.name


def edge_table(t: int) -> np.ndarray:
    bound = max(t + t // 2, 1)                           # (t = 0: the table of bound 1, in which nobody links)
    return edge_targets(bound, EDGE_SEEDS[bound])


def edge_case(t: int, rotations: int = 16) -> Case:
    """(a) the bound's edge: one hub per rotation of the table's candidate order."""
    table = edge_table(t)
    return Case(f"edge-t{t}", t, [np.roll(table, -k) for k in range(rotations)], seed=100 + t)


BLOCK_SIZES = ((1, 2, 31, 32, 33, 63, 64, 65), (511,))    # one library each: the reference's cost grows with the pairs


def block_case(t: int, sizes) -> Case:
    """(b) block and stage edges of the matrix path: one hub per size, all values distinct."""
    bound = t + t // 2
    return Case(f"blocks-t{t}-c" + "-".join(map(str, sizes)), t, [cluster_targets(c, bound, 1000 * t + c) for c in sizes], seed=200 + t)


def dedup_case(t: int, c: int) -> Case:
    """(c) the dedup path just past its entry: a hub of 512 or 513 candidates, 40 distinct values whose probes wrap."""
    return Case(f"dedup-t{t}-c{c}", t, [palette_targets(c, 40, 10 * t + c, collide=True)], endings=True, seed=300 + t)


LIMITS = ((1536, 1536), (1537, 1536), (1537, 1537))     # (candidates, distinct hashes)


def limit_table(t: int, c: int, distinct: int) -> np.ndarray:
    bound = t + t // 2
    table = cluster_targets(distinct, bound, 2000 * t + c + distinct)
    if distinct < c:                                     # one duplicate: the last value once more, at the front
        table = np.concatenate([table[-1:], table])
    assert len(table) == c and len(np.unique(table)) == distinct
    return table


def limit_case(t: int, c: int, distinct: int) -> Case:
    """(c) the dedup table at its limit of 1536 distinct values, and the matrix path's four stages behind it.  Both regions,
    and a spoke holds TWO of the hub's segments, one in each region -- one run per (pair, region) bucket all the same, the
    hub's candidates in target order: 770 videos for 1537 candidates.  (One segment per spoke is 1538 videos, and the
    reference's own per-video pass over all pairs then takes 13 s a library whatever the length of the segments.)"""
    return Case(f"limit-t{t}-c{c}-d{distinct}", t, [limit_table(t, c, distinct)], endings=True,
                per_spoke=[2] * (c // 2) + [1] * (c % 2), seed=400 + t + c + distinct)


SLOT_SHARES = [1] * 40 + [16, 17, 24, 25]


def slot_case(t: int = 10) -> Case:
    """(d) slot edges: behind 40 single spokes, four spokes that share 16, 17, 24 and 25 segments with the hub."""
    return Case(f"slots-t{t}", t, [cluster_targets(sum(SLOT_SHARES), t + t // 2, 77)], per_spoke=SLOT_SHARES, seed=500 + t,
                one_run_per_bucket=False)
