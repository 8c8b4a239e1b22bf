// needle_amd/csrc/pair_ids.h on the CPU: the index store's grouped, append-stable pair numbering (IndexGroupView), the very
// functions the store's kernels run on the device and index.cpp runs on the host.  Against a brute-force enumeration -- video
// after video, its pairs with the earlier videos of its label in list order -- over a few hundred small random label lists
// (0 to 40 videos, 1 to 8 labels, groups interleaved, groups of one) and two hand-made ones (all videos in one group, every
// video alone); and append stability itself: every pair of a prefix of the list has the id it has in the whole list.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "pair_ids.h"

using namespace needle;

static int fail(const char *what, const std::vector<uint32_t> &labels, uint64_t a, uint64_t b) {
  std::printf("FAIL %s: %zu videos, (%llu, %llu); labels", what, labels.size(), (unsigned long long)a, (unsigned long long)b);
  for (size_t v = 0; v < labels.size(); v++) std::printf(" %u", labels[v]);
  std::printf("\n");
  return 1;
}

static uint64_t checked_lists = 0, checked_pairs = 0;

static int check(const std::vector<uint32_t> &labels) {
  const uint32_t n = (uint32_t)labels.size();
  // the numbering by enumeration: column after column, inside a column the lower members in list order
  std::vector<std::pair<uint32_t, uint32_t>> pairs;
  std::vector<uint64_t> id_of((size_t)n * n, ~0ull);  // [a * n + b]
  for (uint32_t b = 0; b < n; b++)
    for (uint32_t a = 0; a < b; a++)
      if (labels[a] == labels[b]) {
        id_of[(size_t)a * n + b] = pairs.size();
        pairs.push_back({a, b});
      }
  const IndexGroupTables tables(labels.data(), n);
  const IndexGroupView t = tables.view();
  if (tables.pairs() != pairs.size() || index_group_pair_count(t) != pairs.size() || t.videos != n)
    return fail("pair count", labels, tables.pairs(), pairs.size());
  // id <-> (a, b): every id hit exactly once
  std::vector<uint32_t> hits(pairs.size(), 0);
  for (uint32_t a = 0; a < n; a++)
    for (uint32_t b = 0; b < n; b++) {
      uint64_t id = ~0ull;
      const bool have = index_group_pair(t, a, b, &id);
      if (have != (a < b && labels[a] == labels[b])) return fail("a pair across groups, or none inside one", labels, a, b);
      if (!have) continue;
      if (id != id_of[(size_t)a * n + b]) return fail("index_group_pair", labels, a, b);
      hits[id]++;
      uint32_t ba = ~0u, bb = ~0u;
      if (!index_group_pair_at(t, id, &ba, &bb) || ba != a || bb != b) return fail("index_group_pair_at", labels, id, ba);
    }
  for (uint64_t p = 0; p < pairs.size(); p++)
    if (hits[p] != 1) return fail("an id not hit exactly once", labels, p, hits[p]);
  uint32_t a = 0, b = 0;
  if (index_group_pair_at(t, pairs.size(), &a, &b) || index_group_pair_at(t, pairs.size() + 1, &a, &b) || index_group_pair_at(t, ~0ull, &a, &b))
    return fail("a pair beyond the last", labels, pairs.size(), 0);
  // one group: the column-major id itself
  if (tables.size.size() == 1)
    for (uint64_t p = 0; p < pairs.size(); p++)
      if (column_major_pair(pairs[p].first, pairs[p].second) != p) return fail("one group is not the column-major numbering", labels, p, 0);
  // a video's slots: the reference's order over the group's sub-list -- the other members in ascending order, the video the
  // destination below its rank and the source above
  for (uint32_t v = 0; v < n; v++) {
    std::vector<uint32_t> partners;
    for (uint32_t m = 0; m < n; m++)
      if (m != v && labels[m] == labels[v]) partners.push_back(m);
    if (index_group_slots(t, v) != partners.size()) return fail("index_group_slots", labels, v, partners.size());
    for (uint32_t q = 0; q < partners.size(); q++) {
      uint32_t sa = ~0u, sb = ~0u;
      const uint64_t id = index_group_slot_pair(t, q, v, &sa, &sb);
      const uint32_t lo = std::min(v, partners[q]), hi = std::max(v, partners[q]);
      if (sa != lo || sb != hi || id != id_of[(size_t)lo * n + hi]) return fail("index_group_slot_pair", labels, v, q);
    }
  }
  // append stability: every pair of every prefix keeps its id, and a prefix's ids are the first ones
  for (uint32_t k = 0; k <= n; k++) {
    const IndexGroupTables prefix(labels.data(), k);
    const IndexGroupView pt = prefix.view();
    if (prefix.pairs() != tables.vbase[k]) return fail("a prefix's ids are not the first ones", labels, k, prefix.pairs());
    for (uint32_t x = 0; x < k; x++) {
      if (pt.rank_of[x] != t.rank_of[x] || pt.vbase[x] != t.vbase[x]) return fail("an append moved a rank or a vbase", labels, k, x);
      for (uint32_t y = x + 1; y < k; y++) {
        uint64_t before = 0, after = 0;
        const bool had = index_group_pair(pt, x, y, &before), has = index_group_pair(t, x, y, &after);
        if (had != has || (had && before != after)) return fail("an append moved an id", labels, x, y);
      }
    }
  }
  checked_lists++;
  checked_pairs += pairs.size();
  return 0;
}

int main() {
  std::mt19937_64 rng(20241020);
  for (int round = 0; round < 400; round++) {
    const size_t n = rng() % 41;
    const uint32_t kinds = 1 + (uint32_t)(rng() % 8);
    std::vector<uint32_t> pool(kinds), labels(n);
    for (uint32_t &x : pool) x = (uint32_t)rng();  // (labels are only compared)
    pool[0] = round & 1 ? 0u : 0xFFFFFFFFu;
    for (uint32_t &x : labels) x = pool[rng() % kinds];
    if (round % 5 == 0 && n > 2) labels[n / 2] = 0x12345678u + (uint32_t)round;  // a video alone among the others
    if (check(labels)) return 1;
  }
  if (check(std::vector<uint32_t>(40, 7u))) return 1;  // all in one group
  std::vector<uint32_t> alone(40);
  for (uint32_t v = 0; v < 40; v++) alone[v] = 1000u - v;  // every video alone: no pair at all
  if (check(alone)) return 1;
  std::printf("%llu label lists, %llu pairs: index group ids ok\n", (unsigned long long)checked_lists, (unsigned long long)checked_pairs);
  return 0;
}
