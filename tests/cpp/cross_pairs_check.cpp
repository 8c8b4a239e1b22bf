// The live-pair table of a grouped cross-matcher (needle_amd/csrc/cross_pairs.h) against brute force, on the CPU: every
// assignment of <= 3 labels to V <= 7 videos, every K <= V - 1 residents, regions 1 and 2.  Checked: the live pairs and their
// order; the two rows; the ids against an independent restatement of the grouped numbering AND against grouped_pair of
// pair_ids.h; the state regions pairwise disjoint, inside the stated total and filling it; the hashes' places likewise; a
// resident without a live pair owning nothing; the byte count; with one label the closed forms of the ungrouped object; every
// refusal as a string.  Prints "cross pairs ok" and the number of cases.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "cross_pairs.h"

using namespace needle;

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::fprintf(stderr, "%s:%d: %s\n  case: %s\n", __FILE__, __LINE__, #cond, g_case.c_str()); \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

static std::string g_case;

// the grouped pair id, restated: groups in the order their first member appears, base = the pairs of the groups before, inside
// a group the i-major order over its members' ranks
static uint64_t brute_id(const std::vector<uint32_t> &labels, size_t a, size_t b) {
  std::vector<uint32_t> order;  // labels in order of first appearance
  for (uint32_t l : labels)
    if (std::find(order.begin(), order.end(), l) == order.end()) order.push_back(l);
  uint64_t base = 0;
  for (uint32_t l : order) {
    const uint64_t n = (uint64_t)std::count(labels.begin(), labels.end(), l);
    if (l == labels[a]) {
      uint64_t ra = 0, rb = 0;
      for (size_t v = 0; v < a; v++) ra += labels[v] == l;
      for (size_t v = 0; v < b; v++) rb += labels[v] == l;
      uint64_t id = base;
      for (uint64_t i = 0; i < ra; i++) id += n - 1 - i;  // the rows before ra
      return id + (rb - ra - 1);
    }
    base += n * (n - 1) / 2;
  }
  return ~0ull;
}

struct Interval {
  uint64_t lo, hi;
};
static void check_disjoint(std::vector<Interval> v, uint64_t from, uint64_t total) {
  std::sort(v.begin(), v.end(), [](const Interval &x, const Interval &y) { return x.lo < y.lo || (x.lo == y.lo && x.hi < y.hi); });
  uint64_t at = from;
  for (const Interval &i : v) {
    if (i.lo == i.hi) continue;  // (an empty row owns nothing)
    CHECK(i.lo >= at && i.hi > i.lo);
    CHECK(i.lo == at);           // ... and nothing is left over between two
    at = i.hi;
  }
  CHECK(at == total);
}

static size_t one_case(const std::vector<uint32_t> &labels, size_t K, size_t R) {
  const size_t V = labels.size(), N = V - K;
  const size_t max_items[2] = {5, 3};
  std::vector<uint32_t> len(K * R);
  for (size_t k = 0; k < K; k++)
    for (size_t r = 0; r < R; r++) len[k * R + r] = (uint32_t)((k * 3 + r * 5 + labels[k]) % 7);  // 0 .. 6, above and below max_items
  CrossPairsShape sh;
  sh.residents = K;
  sh.arriving = N;
  sh.regions = R;
  sh.resident_len = len.data();
  sh.resident_groups = labels.data();
  sh.groups = labels.data() + K;
  sh.max_items = max_items;
  const CrossPairsPlan p = plan_cross_pairs(sh);
  CHECK(p.error == nullptr);
  CHECK(p.labels == labels);

  std::vector<std::pair<size_t, size_t>> want;
  for (size_t t = 0; t < N; t++)
    for (size_t k = 0; k < K; k++)
      if (labels[k] == labels[K + t]) want.push_back({k, K + t});
  const size_t resident_pairs = want.size();
  for (size_t a = K; a < V; a++)
    for (size_t b = a + 1; b < V; b++)
      if (labels[a] == labels[b]) want.push_back({a, b});
  CHECK(p.resident_pairs == resident_pairs && p.arriving_pairs == want.size() - resident_pairs);
  CHECK(p.live.size() == want.size() * R);

  const GroupTables tables(labels.data(), V);
  std::vector<Interval> state, hashes;
  std::vector<uint8_t> live(K, 0);
  uint64_t want_entries = 0;
  bool narrow = true;
  for (size_t q = 0; q < want.size(); q++)
    for (size_t r = 0; r < R; r++) {
      const CrossLive &e = p.live[q * R + r];
      const size_t a = want[q].first, b = want[q].second;
      CHECK(e.row_a == a * R + r && e.row_b == b * R + r);
      uint64_t id = 0;
      CHECK(grouped_pair(tables.view(), (uint32_t)a, (uint32_t)b, &id));
      CHECK(id == brute_id(labels, a, b));
      CHECK(e.problem == id * R + r);
      const uint64_t size = q < resident_pairs ? 2ull * len[a * R + r] : 4ull * max_items[r];
      state.push_back(Interval{e.state, e.state + size});
      want_entries += size;
      if (q < resident_pairs) live[a] = 1;
    }
  CHECK(p.state_entries == want_entries);
  check_disjoint(state, 0, p.state_entries);

  // hashes: the arriving videos' histories, then the live residents' rows; a resident without a live pair owns nothing
  uint64_t want_words = 0;
  for (size_t r = 0; r < R; r++) {
    CHECK(p.hist[r] == want_words);
    for (size_t t = 0; t < N; t++) hashes.push_back(Interval{p.hist[r] + t * max_items[r], p.hist[r] + (t + 1) * max_items[r]});
    want_words += N * max_items[r];
  }
  for (size_t r = 0; r < R; r++) {
    uint64_t region = 0;
    for (size_t k = 0; k < K; k++) {
      CHECK(p.resident_live[k] == live[k]);
      if (!live[k]) continue;
      hashes.push_back(Interval{p.res_hist[r] + p.resident_prefix[k * R + r], p.res_hist[r] + p.resident_prefix[k * R + r] + len[k * R + r]});
      region += len[k * R + r];
      narrow = narrow && len[k * R + r] < 65536;
    }
    CHECK(p.resident_hashes[r] == region);
    want_words += region;
  }
  CHECK(p.hist_words == want_words);
  check_disjoint(hashes, 0, p.hist_words);
  CHECK(p.narrow == narrow);
  CHECK(p.state_bytes() == want_entries * 2 + want_words * 4);

  // one label: the ungrouped object's closed forms (crossmatch.hip ClosedFormPairs)
  if (std::count(labels.begin(), labels.end(), labels[0]) == (long)V) {
    uint64_t S[2] = {0, 0}, prefix[2] = {0, 0};
    for (size_t k = 0; k < K; k++)
      for (size_t r = 0; r < R; r++) S[r] += len[k * R + r];
    std::vector<uint64_t> pre(K * R);
    for (size_t k = 0; k < K; k++)
      for (size_t r = 0; r < R; r++) {
        pre[k * R + r] = prefix[r];
        prefix[r] += len[k * R + r];
      }
    uint64_t at = 0, state_r[2], res_state_r[2];
    for (size_t r = 0; r < R; r++) {
      state_r[r] = at;
      at += (uint64_t)N * (N - 1) / 2 * 4 * max_items[r];
    }
    for (size_t r = 0; r < R; r++) {
      res_state_r[r] = at;
      at += (uint64_t)N * 2 * S[r];
    }
    CHECK(at == p.state_entries);
    for (size_t q = 0; q < want.size(); q++)
      for (size_t r = 0; r < R; r++) {
        const CrossLive &e = p.live[q * R + r];
        const size_t a = want[q].first, b = want[q].second;
        CHECK(e.problem == row_major_pair(a, b, V) * R + r);
        if (q < resident_pairs) {
          CHECK(q == (b - K) * K + a);
          CHECK(e.state == res_state_r[r] + 2 * ((b - K) * S[r] + pre[a * R + r]));
        } else {
          CHECK(e.state == state_r[r] + (q - resident_pairs) * 4 * max_items[r]);
        }
      }
  }
  return 1;
}

static const char *error_of(size_t K, size_t N, size_t R, const uint32_t *len, const uint32_t *res_groups, const uint32_t *groups,
                            const size_t *max_items) {
  CrossPairsShape sh;
  sh.residents = K;
  sh.arriving = N;
  sh.regions = R;
  sh.resident_len = len;
  sh.resident_groups = res_groups;
  sh.groups = groups;
  sh.max_items = max_items;
  const CrossPairsPlan p = plan_cross_pairs(sh);
  if (p.error) {  // a refusal leaves nothing behind
    if (!p.live.empty() || p.state_entries || p.hist_words) return "a refused plan holds a layout";
    return p.error;
  }
  return "";
}

static bool says(const char *got, const char *part) { return got && std::strstr(got, part) != nullptr; }

static void refusals() {
  g_case = "refusals";
  const size_t mi[2] = {8, 8}, small[2] = {1, 8}, large[2] = {8, (size_t)1 << 31};
  std::vector<uint32_t> zeros(70000, 0), lens(70000, 2), distinct(70000);
  for (size_t i = 0; i < distinct.size(); i++) distinct[i] = (uint32_t)i;
  CHECK(says(error_of(0, 2, 0, nullptr, nullptr, zeros.data(), mi), "regions must be 1 or 2"));
  CHECK(says(error_of(0, 2, 3, nullptr, nullptr, zeros.data(), mi), "regions must be 1 or 2"));
  CHECK(says(error_of(0, 2, 1, nullptr, nullptr, nullptr, mi), "null argument"));
  CHECK(says(error_of(0, 2, 1, nullptr, nullptr, zeros.data(), nullptr), "null argument"));
  CHECK(says(error_of(2, 2, 1, nullptr, zeros.data(), zeros.data(), mi), "null argument"));
  CHECK(says(error_of(2, 2, 1, lens.data(), nullptr, zeros.data(), mi), "null argument"));
  CHECK(says(error_of(0, 0, 1, nullptr, nullptr, zeros.data(), mi), "arriving videos must be 1 to 256"));
  CHECK(says(error_of(0, 257, 1, nullptr, nullptr, zeros.data(), mi), "arriving videos must be 1 to 256"));
  CHECK(says(error_of(0, 2, 1, nullptr, nullptr, zeros.data(), small), "max_items must be 2 to 2^31 - 16"));
  CHECK(says(error_of(0, 2, 2, nullptr, nullptr, zeros.data(), large), "max_items must be 2 to 2^31 - 16"));
  std::vector<uint32_t> long_row(2, 0x7FFFFFF1u);
  CHECK(says(error_of(2, 1, 1, long_row.data(), zeros.data(), zeros.data(), mi), "a resident row holds more than"));
  // live problems: the bound is on the same-label pairs with an arriving end, whatever K is
  CHECK(says(error_of(65536, 1, 1, lens.data(), zeros.data(), zeros.data(), mi), "more than 65 535 live problems"));   // exactly 65 536
  CHECK(std::strlen(error_of(65535, 1, 1, lens.data(), zeros.data(), zeros.data(), mi)) == 0);                          // exactly 65 535
  CHECK(says(error_of(32768, 1, 2, lens.data(), zeros.data(), zeros.data(), mi), "more than 65 535 live problems"));   // x 2 regions
  CHECK(says(error_of(255, 256, 1, lens.data(), zeros.data(), zeros.data(), mi), "more than 65 535 live problems"));   // 65 280 + 32 640
  CHECK(std::strlen(error_of(0, 256, 2, nullptr, nullptr, zeros.data(), mi)) == 0);                                     // 65 280
  // ... and the same residents under labels no arriving video has are no live problem at all
  CHECK(std::strlen(error_of(65536, 1, 1, lens.data(), distinct.data() + 1, distinct.data(), mi)) == 0);
  // 300 residents and 256 arriving videos in groups of four: 256 x 1 + 64 x 6 live pairs
  std::vector<uint32_t> res_groups(300), groups(256);
  for (size_t k = 0; k < 300; k++) res_groups[k] = (uint32_t)k;            // one resident each for the first 256 shows ...
  for (size_t t = 0; t < 256; t++) groups[t] = (uint32_t)(t / 4);          // ... of which 64 arrive, four videos each
  CrossPairsShape sh;
  sh.residents = 300;
  sh.arriving = 256;
  sh.regions = 1;
  sh.resident_len = lens.data();
  sh.resident_groups = res_groups.data();
  sh.groups = groups.data();
  sh.max_items = mi;
  const CrossPairsPlan p = plan_cross_pairs(sh);
  CHECK(p.error == nullptr && p.resident_pairs == 256 && p.arriving_pairs == 64 * 6 && p.live.size() == 640);
  CHECK(p.resident_hashes[0] == 64 * 2);  // only the 64 residents whose show arrives own hashes
}

int main() {
  size_t cases = 0;
  for (size_t V = 1; V <= 7; V++) {
    size_t assignments = 1;
    for (size_t v = 0; v < V; v++) assignments *= 3;
    for (size_t code = 0; code < assignments; code++) {
      std::vector<uint32_t> labels(V);
      size_t c = code;
      static const uint32_t kValues[3] = {7u, 0u, 0xFFFFFFFFu};  // (any values: only compared)
      for (size_t v = 0; v < V; v++, c /= 3) labels[v] = kValues[c % 3];
      for (size_t K = 0; K + 1 <= V; K++)
        for (size_t R = 1; R <= 2; R++) {
          g_case = "V=" + std::to_string(V) + " code=" + std::to_string(code) + " K=" + std::to_string(K) + " R=" + std::to_string(R);
          cases += one_case(labels, K, R);
        }
    }
  }
  refusals();
  std::printf("%zu cases\ncross pairs ok\n", cases);
  return 0;
}
