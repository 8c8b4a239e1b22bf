// The live-pair table of a grouped cross-matcher (crossmatch.hip: needle_hip_crossmatcher_new_grouped), built on the host in
// plain C++ -- no HIP types -- so that it can be checked without a device (tests/cpp/cross_pairs_check.cpp).
//
// K resident videos and N arriving ones carry a label each (any 32-bit values: they are only compared); the video list is
// the residents first, V = K + N.  A pair (a, b), a < b, is live where b >= K and the two labels are equal.  The live pairs in
// their order: for every arriving video t its residents k ascending (b = K + t), then the arriving pairs i-major; a live
// problem is live pair * regions + region, which is blockIdx.y of the walk.  With one label this is the ungrouped object's
// order (q = t K + k, then the arriving pairs).
//
// plan_cross_pairs() decides, per live problem, the two rows (video * regions + region over all V), NeedleHipRun.problem
// (grouped_pair of pair_ids.h over the V labels, x regions + region) and where its state lies; and the totals creation
// allocates:
//   hashes: every arriving video's history (max_items[r] words each), then the rows of the residents that are in a live pair,
//           region after region in resident order.  A resident no arriving video shares a label with owns nothing.
//   state:  per region the arriving live pairs' four frontier sets (4 max_items[r] entries each, by the pair's number among
//           the arriving live pairs), then per region the col frontiers of the live (t, k): two sets of len(k, r) entries, at
//           2 x (the lengths of the live residents of the arriving videos before t, plus those of t's own group before k).
// Every refusal is a string in CrossPairsPlan::error.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "pair_ids.h"

namespace needle {

constexpr size_t kCrossMaxArriving = 256;     // arriving videos
constexpr size_t kCrossMaxRegions = 2;
constexpr size_t kCrossMaxLive = 65535;       // live problems: gridDim.y of the walk
constexpr uint64_t kCrossMaxRowItems = 0x7FFFFFF0ull;

// One live problem as crossmatch_walk_kernel's listed policy reads it: uploaded once at creation.
struct CrossLive {
  uint64_t state;          // first entry of its state (an arriving pair: col 0, row 0, col 1, row 1; a resident one: col 0, col 1)
  uint32_t row_a, row_b;   // video * regions + region over all V videos
  uint32_t problem;        // NeedleHipRun.problem
  uint32_t reserved;
};
static_assert(sizeof(CrossLive) == 24, "live-pair table entries are 6 words");

struct CrossPairsShape {
  size_t residents = 0, arriving = 0, regions = 1;
  const uint32_t *resident_len = nullptr;     // residents * regions rows (video k, region r at k * regions + r)
  const uint32_t *resident_groups = nullptr;  // a label per resident
  const uint32_t *groups = nullptr;           // a label per arriving video
  const size_t *max_items = nullptr;          // per region
};

struct CrossPairsPlan {
  const char *error = nullptr;              // null: everything below holds
  std::vector<CrossLive> live;              // live pair q, region r at q * regions + r
  size_t resident_pairs = 0, arriving_pairs = 0;  // live pairs of each kind: resident_pairs of them come first
  std::vector<uint8_t> resident_live;       // per resident: is it in a live pair
  std::vector<uint64_t> resident_prefix;    // per resident row: the region's live resident hashes before it
  uint64_t resident_hashes[2] = {0, 0};     // per region: the live residents' hashes
  uint64_t hist[2] = {0, 0}, res_hist[2] = {0, 0};    // first word of the region's histories / resident hashes
  uint64_t state[2] = {0, 0}, res_state[2] = {0, 0};  // first entry of the region's arriving / resident frontiers
  uint64_t hist_words = 0, state_entries = 0;
  bool narrow = true;                       // u16 entries: every max_items and every live resident row below 65 536
  uint64_t longest_resident = 0;            // row of a live resident
  std::vector<uint32_t> labels;             // of all V videos, residents first

  size_t entry_bytes() const { return narrow ? sizeof(uint16_t) : sizeof(uint32_t); }
  // what creation allocates for frontiers and hashes
  size_t state_bytes() const { return (size_t)(state_entries * entry_bytes() + hist_words * sizeof(uint32_t)); }
};

inline CrossPairsPlan plan_cross_pairs(const CrossPairsShape &sh) {
  CrossPairsPlan p;
  const size_t K = sh.residents, N = sh.arriving, R = sh.regions;
  auto refuse = [&](const char *what) {
    p = CrossPairsPlan();
    p.error = what;
    return p;
  };
  if (R < 1 || R > kCrossMaxRegions) return refuse("crossmatcher: regions must be 1 or 2");
  if (!sh.groups || !sh.max_items || (K && (!sh.resident_len || !sh.resident_groups))) return refuse("crossmatcher: null argument");
  if (N < 1 || N > kCrossMaxArriving) return refuse("crossmatcher: arriving videos must be 1 to 256");
  for (size_t r = 0; r < R; r++)
    if (sh.max_items[r] < 2 || sh.max_items[r] > kCrossMaxRowItems) return refuse("crossmatcher: max_items must be 2 to 2^31 - 16");
  if ((uint64_t)(K + N) * R >= (1ull << 32)) return refuse("crossmatcher: more than 2^32 rows");
  for (size_t i = 0; i < K * R; i++)
    if (sh.resident_len[i] > kCrossMaxRowItems) return refuse("crossmatcher: a resident row holds more than 2^31 - 16 hashes");

  p.labels.assign(sh.resident_groups, sh.resident_groups + K);
  p.labels.insert(p.labels.end(), sh.groups, sh.groups + N);
  const GroupTables tables(p.labels.data(), K + N);
  if (tables.pairs() * R >= (1ull << 32)) return refuse("crossmatcher: the problem index over all videos does not fit 32 bits");
  const GroupView view = tables.view();

  // the live pairs in their order; a group's residents are its members below K, ascending
  struct Pair {
    uint32_t a, b;
  };
  std::vector<Pair> pairs;
  const char *too_many = "crossmatcher: more than 65 535 live problems (same-label pairs with an arriving end x regions)";
  for (size_t t = 0; t < N; t++) {
    const uint32_t g = tables.group_of[K + t], *members = tables.members.data() + tables.first[g];
    for (uint32_t m = 0; m < tables.size[g] && members[m] < K; m++) {
      pairs.push_back(Pair{members[m], (uint32_t)(K + t)});
      if (pairs.size() * R > kCrossMaxLive) return refuse(too_many);
    }
  }
  p.resident_pairs = pairs.size();
  for (size_t ta = 0; ta < N; ta++) {
    const uint32_t g = tables.group_of[K + ta], *members = tables.members.data() + tables.first[g];
    for (uint32_t m = tables.rank_of[K + ta] + 1; m < tables.size[g]; m++) {
      pairs.push_back(Pair{(uint32_t)(K + ta), members[m]});
      if (pairs.size() * R > kCrossMaxLive) return refuse(too_many);
    }
  }
  p.arriving_pairs = pairs.size() - p.resident_pairs;

  // which residents are live, and where their hashes lie
  p.resident_live.assign(K, 0);
  for (size_t q = 0; q < p.resident_pairs; q++) p.resident_live[pairs[q].a] = 1;
  p.resident_prefix.assign(K * R, 0);
  for (size_t k = 0; k < K; k++)
    for (size_t r = 0; r < R; r++) {
      p.resident_prefix[k * R + r] = p.resident_hashes[r];
      if (!p.resident_live[k]) continue;
      const uint64_t len = sh.resident_len[k * R + r];
      p.resident_hashes[r] += len;
      p.narrow = p.narrow && len < 65536;
      if (len > p.longest_resident) p.longest_resident = len;
    }
  for (size_t r = 0; r < R; r++) {
    p.narrow = p.narrow && sh.max_items[r] < 65536;
    p.hist[r] = p.hist_words;
    p.state[r] = p.state_entries;
    p.hist_words += (uint64_t)N * sh.max_items[r];
    p.state_entries += (uint64_t)p.arriving_pairs * 4 * sh.max_items[r];
  }
  for (size_t r = 0; r < R; r++) {
    p.res_hist[r] = p.hist_words;
    p.hist_words += p.resident_hashes[r];
  }

  // the table: the resident pairs' col frontiers pair after pair (t-major, so a per-t prefix over t's own group's residents),
  // region after region
  p.live.resize(pairs.size() * R);
  for (size_t r = 0; r < R; r++) {
    p.res_state[r] = p.state_entries;
    for (size_t q = 0; q < pairs.size(); q++) {
      const Pair pr = pairs[q];
      uint64_t id = 0;
      (void)grouped_pair(view, pr.a, pr.b, &id);  // (of one group by construction)
      CrossLive &e = p.live[q * R + r];
      e.row_a = (uint32_t)(pr.a * R + r);
      e.row_b = (uint32_t)(pr.b * R + r);
      e.problem = (uint32_t)(id * R + r);
      e.reserved = 0;
      if (q < p.resident_pairs) {
        e.state = p.state_entries;
        p.state_entries += 2 * (uint64_t)sh.resident_len[pr.a * R + r];
      } else {
        e.state = p.state[r] + (uint64_t)(q - p.resident_pairs) * 4 * sh.max_items[r];
      }
    }
  }
  return p;
}

}  // namespace needle
