// The host plan of every cross-matcher (crossmatch.hip executes it): which problems are live, what each one is called and
// where everything lies, in plain C++ -- no HIP types -- so that it can be checked without a device
// (tests/cpp/cross_pairs_check.cpp).
//
// K resident videos (complete at creation) and N arriving ones (the lanes); the video list is the residents first, V = K + N.
// With labels every video carries one (any 32-bit values: they are only compared) and a pair (a, b), a < b, is live where
// b >= K and the two labels are equal; without labels (`groups` null) the object is planned as one label: every pair with an
// arriving end.  The live pairs in their order: for every arriving video t its residents k ascending (b = K + t), then the
// arriving pairs i-major; a live problem is live pair * regions + region, which is blockIdx.y of the walk.  With one label
// that is q = t K + k, then the arriving pairs as the comparator numbers them: the walk of an unlabelled object finds it by
// arithmetic (ClosedFormPairs) and no table is uploaded.
//
// plan_cross_pairs() decides, per live problem, the two rows (video * regions + region over all V), NeedleHipRun.problem
// (grouped_pair of pair_ids.h over the V labels, x regions + region; one label: the comparator's i-major index) and where its
// state lies; and the one layout of all the objects:
//   hashes: every arriving video's history (max_items[r] words each) region after region, then the rows of the residents that
//           are in a live pair, region after region in resident order (res_hist[r] + resident_prefix).  A resident no arriving
//           video shares a label with owns nothing.
//   state:  per region the arriving live pairs' four frontier sets (col 0, row 0, col 1, row 1: 4 max_items[r] entries, by the
//           pair's number among the arriving live pairs, from state[r]), then per region from res_state[r] the col frontiers
//           of the live (t, k): two sets of len(k, r) entries, at 2 x (the lengths of the live residents of the arriving
//           videos before t, plus those of t's own group before k) -- with one label 2 x (t S_r + prefix(k, r)), S_r =
//           resident_hashes[r].  Entries are u16 where every max_items and every live resident row is below 65 536, else u32.
// Every refusal is a string in CrossPairsPlan::error.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/needle_hip.h"
#include "pair_ids.h"

namespace needle {

constexpr size_t kCrossMaxArriving = 256;     // arriving videos: 32 640 pairs x 2 regions = 65 280 <= kCrossMaxLive
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

// What a cross-matcher is made from (CrossMatcher::Spec).
struct CrossPairsShape {
  size_t residents = 0, arriving = 0, regions = 1;
  const NeedleHipSeq *resident = nullptr;     // residents * regions rows of the caller's arena (video k, region r at k * regions + r)
  const uint32_t *resident_groups = nullptr;  // a label per resident; not read without `groups`
  const uint32_t *groups = nullptr;           // a label per arriving video; null: the unlabelled object
  const size_t *max_items = nullptr;          // per region
  const uint32_t *min_len = nullptr;          // per region; null (a question about sizes): not checked
  uint64_t arena_hashes = ~0ull;              // the arena's size: every resident row lies inside (the default: nothing to check)
  uint32_t threshold = 0;
};

struct CrossPairsPlan {
  const char *error = nullptr;              // null: everything below holds
  bool labelled = false;
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
  std::vector<uint32_t> labels;             // of all V videos, residents first; empty without labels
  std::unique_ptr<const GroupTables> tables;  // pair_ids.h over the V labels (one label without)
  // the groups that arrive, numbered as they first do: per arriving video its group, and per group and region the sum over
  // the group's resident rows of max(len, 1) - 1
  size_t regions = 1;
  std::vector<uint32_t> lane_group;
  std::vector<uint64_t> resident_cell_rows;

  size_t problems() const { return (resident_pairs + arriving_pairs) * regions; }
  size_t entry_bytes() const { return narrow ? sizeof(uint16_t) : sizeof(uint32_t); }
  // what creation allocates for frontiers and hashes
  size_t state_bytes() const { return (size_t)(state_entries * entry_bytes() + hist_words * sizeof(uint32_t)); }

  // The two videos (of all V) and the region of NeedleHipRun.problem; false where no pair has that id.
  bool problem_at(uint32_t problem, uint32_t *a, uint32_t *b, uint32_t *r) const {
    *r = (uint32_t)(problem % regions);
    return grouped_pair_at(tables->view(), problem / regions, a, b);
  }

  // Cells of all live problems where lane i = arriving video * regions + region has x_of(i) = max(items, 1) - 1 rows of
  // cells: x_a x_b summed over the live problems' two rows, which per group and region is (S^2 - Q) / 2 + Rg S -- S and Q
  // the sum of the group's arriving x and of their squares, Rg its resident rows'.  O(lanes): no walk over the live problems.
  template <class X>
  uint64_t cells(X x_of) const {
    uint64_t sum[kCrossMaxArriving * kCrossMaxRegions], squares[kCrossMaxArriving * kCrossMaxRegions], total = 0;
    std::fill(sum, sum + resident_cell_rows.size(), 0);
    std::fill(squares, squares + resident_cell_rows.size(), 0);
    for (size_t t = 0, i = 0; t < lane_group.size(); t++)
      for (size_t r = 0; r < regions; r++, i++) {
        const uint64_t x = x_of(i);
        const size_t at = lane_group[t] * regions + r;
        sum[at] += x;
        squares[at] += x * x;
      }
    for (size_t at = 0; at < resident_cell_rows.size(); at++) total += (sum[at] * sum[at] - squares[at]) / 2 + resident_cell_rows[at] * sum[at];
    return total;
  }
};

inline CrossPairsPlan plan_cross_pairs(const CrossPairsShape &sh) {
  CrossPairsPlan p;
  const size_t K = sh.residents, N = sh.arriving, R = sh.regions;
  const bool labelled = sh.groups != nullptr;
  auto refuse = [&](const char *what) {
    p = CrossPairsPlan();
    p.error = what;
    return std::move(p);
  };
  const char *too_many = labelled ? "crossmatcher: more than 65 535 live problems (same-label pairs with an arriving end x regions)"
                                  : "crossmatcher: more than 65 535 live problems ((K N + N (N - 1) / 2) x regions)";
  const char *too_wide = "crossmatcher: the problem index over all videos does not fit 32 bits";
  if (R < 1 || R > kCrossMaxRegions) return refuse("crossmatcher: regions must be 1 or 2");
  if (!sh.max_items || (K && (!sh.resident || (labelled && !sh.resident_groups)))) return refuse("crossmatcher: null argument");
  if (!labelled && !K && (N < 2 || N > kCrossMaxArriving)) return refuse("crossmatcher: lanes (videos) must be 2 to 256");
  if (N < 1 || N > kCrossMaxArriving) return refuse("crossmatcher: arriving videos must be 1 to 256");
  for (size_t r = 0; r < R; r++)
    if (sh.max_items[r] < 2 || sh.max_items[r] > kCrossMaxRowItems) return refuse("crossmatcher: max_items must be 2 to 2^31 - 16");
  if (!labelled) {  // every pair is live: the two bounds by arithmetic on K and N, before a row is read or anything is allocated
    if (K > kCrossMaxLive || (K * N + N * (N - 1) / 2) * R > kCrossMaxLive) return refuse(too_many);
    if ((uint64_t)(K + N) * (K + N - 1) / 2 * R >= (1ull << 32)) return refuse(too_wide);
  } else if ((uint64_t)(K + N) * R >= (1ull << 32)) {
    return refuse("crossmatcher: more than 2^32 rows");
  }
  auto outside = [&](size_t i) { return (uint64_t)sh.resident[i].offset + sh.resident[i].len > sh.arena_hashes; };
  const char *outside_arena = "crossmatcher: a resident row lies outside the hash arena";
  for (size_t i = 0; i < K * R; i++) {
    if (sh.resident[i].len > kCrossMaxRowItems) return refuse("crossmatcher: a resident row holds more than 2^31 - 16 hashes");
    if (!labelled && outside(i)) return refuse(outside_arena);  // (with labels the arena is the last refusal)
  }
  auto min_len_is_zero = [&] { return sh.min_len && (sh.min_len[0] == 0 || sh.min_len[R - 1] == 0); };
  const char *zero_min_len = "crossmatcher: min_len must be >= 1";
  if (!labelled && min_len_is_zero()) return refuse(zero_min_len);  // (the last refusal without labels: nothing sized by K before it)

  std::vector<uint32_t> labels(K + N, 0u);
  if (labelled) {
    std::copy(sh.resident_groups, sh.resident_groups + K, labels.begin());
    std::copy(sh.groups, sh.groups + N, labels.begin() + K);
  }
  p.tables.reset(new GroupTables(labels.data(), K + N));
  const GroupTables &tables = *p.tables;
  if (tables.pairs() * R >= (1ull << 32)) return refuse(too_wide);
  const GroupView view = tables.view();

  // the live pairs in their order; a group's residents are its members below K, ascending
  struct Pair {
    uint32_t a, b;
  };
  std::vector<Pair> pairs;
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
  if (min_len_is_zero()) return refuse(zero_min_len);
  for (size_t i = 0; i < K * R && labelled; i++)
    if (outside(i)) return refuse(outside_arena);
  p.labelled = labelled;
  p.regions = R;
  if (labelled) p.labels.swap(labels);

  // the groups that arrive, and what their residents add to the cells
  std::vector<uint32_t> arriving_group(tables.size.size(), ~0u);
  p.lane_group.resize(N);
  for (size_t t = 0; t < N; t++) {
    uint32_t &dense = arriving_group[tables.group_of[K + t]];
    if (dense == ~0u) {
      dense = (uint32_t)(p.resident_cell_rows.size() / R);
      p.resident_cell_rows.resize(p.resident_cell_rows.size() + R, 0);
    }
    p.lane_group[t] = dense;
  }

  // which residents are live, and where their hashes lie
  p.resident_live.assign(K, 0);
  p.resident_prefix.assign(K * R, 0);
  for (size_t k = 0; k < K; k++)
    for (size_t r = 0; r < R; r++) {
      p.resident_prefix[k * R + r] = p.resident_hashes[r];
      const uint32_t dense = arriving_group[tables.group_of[k]];
      if (dense == ~0u) continue;
      p.resident_live[k] = 1;
      const uint64_t len = sh.resident[k * R + r].len;
      p.resident_hashes[r] += len;
      p.resident_cell_rows[dense * R + r] += std::max<uint64_t>(len, 1) - 1;
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
        p.state_entries += 2 * (uint64_t)sh.resident[pr.a * R + r].len;
      } else {
        e.state = p.state[r] + (uint64_t)(q - p.resident_pairs) * 4 * sh.max_items[r];
      }
    }
  }
  return p;
}

}  // namespace needle
