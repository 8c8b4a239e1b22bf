// The two pair numberings and the way from one to the other, for the host and the device alike (tests/cpp/pair_ids_check.cpp
// runs these very functions on the CPU).  Every intermediate is 64-bit: V (V - 1) / 2 x regions may come close to 2^32.
//   i-major (the comparator's, NeedleHipRun.problem of a cross-matcher over V videos): pair (a, b), a < b, is
//     a (2 V - a - 1) / 2 + (b - a - 1); it depends on V.
//   column-major (the index store's): p(a, b) = b (b - 1) / 2 + a; it does not, so an append adds ids at the end.
//   grouped (a library of many seasons, further down): only pairs inside one group of videos have an id.
//   grouped and append-stable (the grouped index's store, the end of this file): the column-major id over groups.
#pragma once

#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEEDLE_HOST_DEVICE __host__ __device__
#else
#define NEEDLE_HOST_DEVICE
#endif

namespace needle {

// first i-major pair of row a: the rows before it hold (V - 1) + (V - 2) + ... + (V - a) pairs
NEEDLE_HOST_DEVICE inline uint64_t row_major_start(uint64_t a, uint64_t V) { return a * (2 * V - a - 1) / 2; }
NEEDLE_HOST_DEVICE inline uint64_t row_major_pair(uint64_t a, uint64_t b, uint64_t V) { return row_major_start(a, V) + (b - a - 1); }
NEEDLE_HOST_DEVICE inline uint64_t column_major_pair(uint64_t a, uint64_t b) { return b * (b - 1) / 2 + a; }

// (a, b) of i-major pair `pair` over V videos; false where there is no such pair.  The last row that starts at or before
// `pair`, by bisection: exact, no floating point.
NEEDLE_HOST_DEVICE inline bool row_major_pair_at(uint64_t pair, uint64_t V, uint32_t *a, uint32_t *b) {
  if (V < 2 || pair >= V * (V - 1) / 2) return false;
  uint64_t lo = 0, hi = V - 2;
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) / 2;
    if (row_major_start(mid, V) <= pair) lo = mid;
    else hi = mid - 1;
  }
  *a = (uint32_t)lo;
  *b = (uint32_t)(lo + 1 + (pair - row_major_start(lo, V)));
  return true;
}

// problem = i-major pair * regions + region -> (a, b, region)
NEEDLE_HOST_DEVICE inline bool decode_problem(uint32_t problem, uint32_t regions, uint64_t V, uint32_t *a, uint32_t *b, uint32_t *r) {
  if (regions == 0) return false;
  *r = problem % regions;
  return row_major_pair_at(problem / regions, V, a, b);
}

// The tag of (a, b, region) in an append onto n0 videos (b >= n0): the store's bucket less the append's first one, p(0, n0).
NEEDLE_HOST_DEVICE inline uint64_t append_tag(uint64_t a, uint64_t b, uint64_t r, uint64_t n0, uint64_t regions) {
  const uint64_t first = n0 ? column_major_pair(0, n0) : 0;
  return (column_major_pair(a, b) - first) * regions + r;
}

// ---- grouped: videos carry a label, equal labels are one season, and only pairs inside a season exist --------------------
// Groups are numbered g = 0, 1, ... in the order their first member appears in the list; a group's members are its list
// positions in ascending order (they need not be adjacent), n_g of them, and a member's rank is its index among them.
// base[g] = sum over h < g of n_h (n_h - 1) / 2, and pair (a, b), a < b, both of group g with ranks (ra, rb), is
// base[g] + row_major_pair(ra, rb, n_g): inside a group the reference's own order over that group's sub-list, so one group
// is the i-major numbering.  The tables as pointers, in host or in device memory:
struct GroupView {
  const uint32_t *group_of, *rank_of;  // per video
  const uint32_t *size, *first;        // per group: n_g, where its members start in `members`
  const uint64_t *base;                // per group, and base[num_groups] = all grouped pairs
  const uint32_t *members;             // list positions, group after group
  uint32_t num_groups;
};

NEEDLE_HOST_DEVICE inline uint64_t grouped_pair_count(const GroupView &t) { return t.base[t.num_groups]; }

// id of (a, b), a < b; false where the two are not of one group
NEEDLE_HOST_DEVICE inline bool grouped_pair(const GroupView &t, uint32_t a, uint32_t b, uint64_t *pair) {
  const uint32_t g = t.group_of[a];
  if (a >= b || t.group_of[b] != g) return false;
  *pair = t.base[g] + row_major_pair(t.rank_of[a], t.rank_of[b], t.size[g]);
  return true;
}

// (a, b) of grouped pair `pair`; false where there is no such pair.  The last group whose base is at or before `pair` (a
// group without pairs shares its base with the next one, so that is the group that holds it), by bisection.
NEEDLE_HOST_DEVICE inline bool grouped_pair_at(const GroupView &t, uint64_t pair, uint32_t *a, uint32_t *b) {
  if (t.num_groups == 0 || pair >= grouped_pair_count(t)) return false;
  uint32_t lo = 0, hi = t.num_groups - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (t.base[mid] <= pair) lo = mid;
    else hi = mid - 1;
  }
  uint32_t ra, rb;
  if (!row_major_pair_at(pair - t.base[lo], t.size[lo], &ra, &rb)) return false;
  *a = t.members[t.first[lo] + ra];
  *b = t.members[t.first[lo] + rb];
  return true;
}

// a video's pairs: n_g - 1 slots, in the reference's order over its group -- (q-th lower member, v), then (v, higher member)
NEEDLE_HOST_DEVICE inline uint32_t grouped_slots(const GroupView &t, uint32_t v) { return t.size[t.group_of[v]] - 1; }
NEEDLE_HOST_DEVICE inline uint64_t grouped_rank_slot_pair(uint64_t base, uint64_t rank, uint64_t size, uint64_t q) {
  return base + (q < rank ? row_major_pair(q, rank, size) : row_major_pair(rank, q + 1, size));
}
NEEDLE_HOST_DEVICE inline uint64_t grouped_slot_pair(const GroupView &t, uint32_t q, uint32_t v, uint32_t *a, uint32_t *b) {
  const uint32_t g = t.group_of[v], rank = t.rank_of[v];
  const uint32_t other = t.members[t.first[g] + (q < rank ? q : q + 1)];
  *a = q < rank ? other : v;
  *b = q < rank ? v : other;
  return grouped_rank_slot_pair(t.base[g], rank, t.size[g], q);
}

// The tables of one call, built once on the host from the labels (any values: they are only compared).
struct GroupTables {
  std::vector<uint32_t> group_of, rank_of, size, first, members;
  std::vector<uint64_t> base;
  GroupTables(const uint32_t *labels, size_t n) : group_of(n), rank_of(n), members(n) {
    std::unordered_map<uint32_t, uint32_t> seen;
    for (size_t v = 0; v < n; v++) {
      const auto at = seen.emplace(labels[v], (uint32_t)size.size());
      if (at.second) size.push_back(0);
      group_of[v] = at.first->second;
      rank_of[v] = size[group_of[v]]++;
    }
    first.resize(size.size());
    base.resize(size.size() + 1);
    uint64_t pairs = 0;
    uint32_t at = 0;
    for (size_t g = 0; g < size.size(); g++) {
      base[g] = pairs;
      first[g] = at;
      pairs += (uint64_t)size[g] * (size[g] - 1) / 2;
      at += size[g];
    }
    base[size.size()] = pairs;
    for (size_t v = 0; v < n; v++) members[first[group_of[v]] + rank_of[v]] = (uint32_t)v;
  }
  uint64_t pairs() const { return base.back(); }
  GroupView view() const {
    return GroupView{group_of.data(), rank_of.data(), size.data(), first.data(), base.data(), members.data(), (uint32_t)size.size()};
  }
};

// ---- grouped and append-stable: the index store's numbering of a library of many seasons ----------------------------------
// base[g] above moves when an earlier group grows, so a store that is appended to cannot keep it.  The column-major id,
// generalised: vbase[v] = sum over u < v of rank_of[u], and pair (a, b), a < b, both of one group, is vbase[b] + rank_of[a] --
// video b's column holds its pairs with the lower-ranked members of its group, rank_of[b] of them.  A video appended to the
// list changes no rank and no vbase of a video already present, so it adds ids only at the end; with one group the rank is the
// position and the id is column_major_pair(a, b).  Groups, ranks and members are GroupTables'.
struct IndexGroupView {
  const uint32_t *group_of, *rank_of;  // per video
  const uint32_t *size, *first;        // per group: n_g, where its members start in `members`
  const uint32_t *members;             // list positions, group after group
  const uint64_t *vbase;               // per video, and vbase[videos] = all pairs
  uint32_t videos;
};

NEEDLE_HOST_DEVICE inline uint64_t index_group_pair_count(const IndexGroupView &t) { return t.vbase[t.videos]; }

// id of (a, b), a < b; false where the two are not of one group
NEEDLE_HOST_DEVICE inline bool index_group_pair(const IndexGroupView &t, uint32_t a, uint32_t b, uint64_t *pair) {
  if (a >= b || b >= t.videos || t.group_of[a] != t.group_of[b]) return false;
  *pair = t.vbase[b] + t.rank_of[a];
  return true;
}

// (a, b) of pair `pair`; false where there is no such pair.  The last video whose vbase is at or before `pair`, by bisection (a
// video of rank 0 has no column and shares its vbase with the next video, so that is the video that holds it).
NEEDLE_HOST_DEVICE inline bool index_group_pair_at(const IndexGroupView &t, uint64_t pair, uint32_t *a, uint32_t *b) {
  if (t.videos == 0 || pair >= index_group_pair_count(t)) return false;
  uint32_t lo = 0, hi = t.videos - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (t.vbase[mid] <= pair) lo = mid;
    else hi = mid - 1;
  }
  const uint64_t ra = pair - t.vbase[lo];
  if (ra >= t.rank_of[lo]) return false;
  *a = t.members[t.first[t.group_of[lo]] + ra];
  *b = lo;
  return true;
}

// a video's pairs: n_g - 1 slots, in the reference's order over its group.  Slot q below v's rank is (q-th member, v), in v's
// own column; a slot at or above it is (v, member q + 1), in that member's column.
NEEDLE_HOST_DEVICE inline uint32_t index_group_slots(const IndexGroupView &t, uint32_t v) { return t.size[t.group_of[v]] - 1; }
NEEDLE_HOST_DEVICE inline uint64_t index_group_slot_pair(const IndexGroupView &t, uint32_t q, uint32_t v, uint32_t *a, uint32_t *b) {
  const uint32_t rank = t.rank_of[v];
  const uint32_t other = t.members[t.first[t.group_of[v]] + (q < rank ? q : q + 1)];
  *a = q < rank ? other : v;
  *b = q < rank ? v : other;
  return q < rank ? t.vbase[v] + q : t.vbase[other] + rank;
}

// The tables of an index's current list, built on the host at every operation (a few words per video).
struct IndexGroupTables : GroupTables {
  std::vector<uint64_t> vbase;
  IndexGroupTables(const uint32_t *labels, size_t n) : GroupTables(labels, n), vbase(n + 1) {
    uint64_t pairs = 0;
    for (size_t v = 0; v < n; v++) {
      vbase[v] = pairs;
      pairs += rank_of[v];
    }
    vbase[n] = pairs;
  }
  uint64_t pairs() const { return vbase.back(); }
  IndexGroupView view() const {
    return IndexGroupView{group_of.data(), rank_of.data(), size.data(), first.data(), members.data(), vbase.data(), (uint32_t)group_of.size()};
  }
};

}  // namespace needle
