// needle_amd/csrc/pair_ids.h on the CPU: the grouped pair numbering, the very functions GroupedPairs / GroupedVideos run on the
// device and the host epilogue runs per pair.  Against the enumeration itself -- groups in order of first appearance, inside a
// group the i-major order over its members -- for every partition of up to 7 videos into groups (labels drawn from a table
// that holds 0 and 0xFFFFFFFF) and a few hundred random label vectors of up to 600 videos: interleaved members, groups of one,
// one group of 258 (past the 256 slots best_match_kernel takes at a time).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "pair_ids.h"

using namespace needle;

static int fail(const char *what, const std::vector<uint32_t> &labels, uint64_t a, uint64_t b) {
  std::printf("FAIL %s: %zu videos, pair / slot (%llu, %llu); labels", what, labels.size(), (unsigned long long)a, (unsigned long long)b);
  for (size_t v = 0; v < labels.size() && v < 32; v++) std::printf(" %u", labels[v]);
  std::printf("\n");
  return 1;
}

static uint64_t checked_vectors = 0, checked_pairs = 0;

static int check(const std::vector<uint32_t> &labels) {
  const size_t n = labels.size();
  // the numbering by enumeration
  std::vector<uint32_t> order;  // labels in order of first appearance
  std::map<uint32_t, std::vector<uint32_t>> members;
  for (size_t v = 0; v < n; v++) {
    if (!members.count(labels[v])) order.push_back(labels[v]);
    members[labels[v]].push_back((uint32_t)v);
  }
  std::vector<std::pair<uint32_t, uint32_t>> pairs;
  std::vector<uint32_t> id_of(n * n, 0);  // [a * n + b]
  for (uint32_t label : order) {
    const std::vector<uint32_t> &m = members[label];
    for (size_t x = 0; x < m.size(); x++)
      for (size_t y = x + 1; y < m.size(); y++) {
        id_of[m[x] * n + m[y]] = (uint32_t)pairs.size();
        pairs.push_back({m[x], m[y]});
      }
  }
  const GroupTables tables(labels.data(), n);
  const GroupView t = tables.view();
  if (tables.pairs() != pairs.size() || grouped_pair_count(t) != pairs.size() || t.num_groups != order.size())
    return fail("pair or group count", labels, tables.pairs(), pairs.size());
  // id <-> (a, b), dense in [0, sum n_g (n_g - 1) / 2)
  for (uint64_t p = 0; p < pairs.size(); p++) {
    uint32_t a = ~0u, b = ~0u;
    uint64_t back = ~0ull;
    if (!grouped_pair_at(t, p, &a, &b) || a != pairs[p].first || b != pairs[p].second) return fail("grouped_pair_at", labels, p, a);
    if (!grouped_pair(t, a, b, &back) || back != p) return fail("grouped_pair", labels, a, b);
  }
  uint32_t a = 0, b = 0;
  if (grouped_pair_at(t, pairs.size(), &a, &b) || grouped_pair_at(t, pairs.size() + 1, &a, &b) || grouped_pair_at(t, ~0ull, &a, &b))
    return fail("a pair beyond the last", labels, pairs.size(), 0);
  for (uint32_t x = 0; x < n; x++)
    for (uint32_t y = 0; y < n && n <= 64; y++) {  // (all ordered pairs while that is cheap)
      uint64_t id = 0;
      const bool have = grouped_pair(t, x, y, &id);
      if (have != (x < y && labels[x] == labels[y])) return fail("a pair across groups, or none inside one", labels, x, y);
    }
  if (order.size() == 1)
    for (uint64_t p = 0; p < pairs.size(); p++)
      if (row_major_pair(pairs[p].first, pairs[p].second, n) != p) return fail("one group is not the i-major numbering", labels, p, 0);
  // a video's slots: its group's other members in ascending order, itself the destination below its rank and the source above
  for (uint32_t v = 0; v < n; v++) {
    std::vector<uint32_t> partners;
    for (uint32_t m : members[labels[v]])
      if (m != v) partners.push_back(m);
    if (grouped_slots(t, v) != partners.size()) return fail("grouped_slots", labels, v, partners.size());
    for (uint32_t q = 0; q < partners.size(); q++) {
      uint32_t sa = ~0u, sb = ~0u;
      const uint64_t id = grouped_slot_pair(t, q, v, &sa, &sb);
      const uint32_t lo = std::min(v, partners[q]), hi = std::max(v, partners[q]);
      if (sa != lo || sb != hi || id != id_of[lo * n + hi]) return fail("grouped_slot_pair", labels, v, q);
      const uint32_t g = t.group_of[v];
      if (grouped_rank_slot_pair(t.base[g], t.rank_of[v], t.size[g], q) != id) return fail("grouped_rank_slot_pair", labels, v, q);
    }
  }
  checked_vectors++;
  checked_pairs += pairs.size();
  return 0;
}

int main() {
  // every partition of n <= 7 videos: restricted-growth strings, a group's index mapped to a label that says nothing about it
  const uint32_t names[7] = {0xFFFFFFFFu, 7u, 0u, 0x80000000u, 3u, 0x7FFFFFFFu, 1u};
  for (size_t n = 0; n <= 7; n++) {
    std::vector<uint32_t> rgs(n, 0), labels(n);
    for (;;) {
      for (size_t v = 0; v < n; v++) labels[v] = names[rgs[v]];
      if (check(labels)) return 1;
      // next restricted-growth string: the last position that may still grow
      size_t k = n;
      while (k-- > 1) {
        uint32_t most = 0;
        for (size_t x = 0; x < k; x++) most = std::max(most, rgs[x]);
        if (rgs[k] <= most) break;
      }
      if (n < 2 || k == 0) break;
      rgs[k]++;
      for (size_t x = k + 1; x < n; x++) rgs[x] = 0;
    }
  }
  if (checked_vectors != 1 + 1 + 2 + 5 + 15 + 52 + 203 + 877) {  // the Bell numbers
    std::printf("FAIL: %llu partitions walked\n", (unsigned long long)checked_vectors);
    return 1;
  }
  // random label vectors of up to 600 videos: few or many groups, labels anywhere in 32 bits
  std::mt19937_64 rng(20240229);
  for (int round = 0; round < 300; round++) {
    const size_t n = 1 + rng() % 600;
    const uint32_t kinds = 1 + (uint32_t)(rng() % (round % 3 == 0 ? 4 : round % 3 == 1 ? 40 : n));
    std::vector<uint32_t> pool(kinds), labels(n);
    for (uint32_t &x : pool) x = (uint32_t)rng();
    pool[0] = round & 1 ? 0u : 0xFFFFFFFFu;
    for (uint32_t &x : labels) x = pool[rng() % kinds];
    if (check(labels)) return 1;
  }
  {  // one group of 258 interleaved with a group of 5 and two videos alone
    std::vector<uint32_t> labels;
    for (uint32_t v = 0; v < 258; v++) {
      labels.push_back(0xFFFFFFFFu);
      if (v % 60 == 7) labels.push_back(0u);
      if (v == 100 || v == 257) labels.push_back(1000u + v);
    }
    if (std::count(labels.begin(), labels.end(), 0xFFFFFFFFu) != 258 || std::count(labels.begin(), labels.end(), 0u) != 5) return fail("the 258", labels, 0, 0);
    if (check(labels)) return 1;
  }
  std::printf("%llu label vectors, %llu pairs: group ids ok\n", (unsigned long long)checked_vectors, (unsigned long long)checked_pairs);
  return 0;
}
