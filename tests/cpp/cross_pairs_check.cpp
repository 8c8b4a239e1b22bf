// The host plan of every cross-matcher (needle_amd/csrc/cross_pairs.h) on the CPU.
// Against brute force: every assignment of <= 3 labels to V <= 7 videos, every K <= V - 1 residents, regions 1 and 2.  Checked:
// the live pairs and their order; the two rows; the ids against an independent restatement of the grouped numbering AND against
// grouped_pair of pair_ids.h; the state regions pairwise disjoint, inside the stated total and filling it; the hashes' places
// likewise; a resident without a live pair owning nothing; the byte count; with one label the closed forms of the unlabelled
// object's walk; the cells of a round (CrossPairsPlan::cells) against the sum over the live problems at two sets of lane fill
// levels; the host's decode of NeedleHipRun.problem (CrossPairsPlan::problem_at) for every live problem; every refusal as a
// string.
// Against the object without labels as it was before one plan served both (namespace before: its argument checks, its layout
// loop and its byte count, verbatim): the plan of a shape without labels agrees field by field for every K <= 4, N <= 5,
// regions 1 and 2 and row lengths that include 0 and 1, and refusal by refusal at the boundary shapes.
// Prints the number of cases and "cross pairs ok".
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

// rows of these lengths, one after the other in an arena
static std::vector<NeedleHipSeq> rows_of(const std::vector<uint32_t> &len) {
  std::vector<NeedleHipSeq> rows(len.size());
  uint32_t at = 0;
  for (size_t i = 0; i < len.size(); i++) {
    rows[i] = NeedleHipSeq{at, len[i]};
    at += len[i];  // (may wrap where a test asks for rows no arena holds: nothing reads the offsets then)
  }
  return rows;
}

// The cells of a round and the decode of a problem, for any plan: lane i holds fill[i] items.
static void check_cells_and_decode(const CrossPairsPlan &p, const std::vector<CrossLive> &live, const std::vector<uint32_t> &len, size_t K,
                                   size_t N, size_t R) {
  for (size_t level = 0; level < 2; level++) {
    std::vector<uint64_t> x(N * R);  // max(items, 1) - 1; the first level leaves lanes empty and at one item
    for (size_t i = 0; i < x.size(); i++) x[i] = level == 0 ? (i % 3 == 0 ? 0 : (i * 7 + 2) % 5) : (i * 5 + 3) % 11 + (i % 4 == 1 ? 0 : 1);
    auto x_of_row = [&](size_t row) -> uint64_t { return row < K * R ? std::max<uint64_t>(len[row], 1) - 1 : x[row - K * R]; };
    uint64_t want = 0;
    for (const CrossLive &e : live) want += x_of_row(e.row_a) * x_of_row(e.row_b);
    CHECK(p.cells([&](size_t i) { return x[i]; }) == want);
  }
  for (const CrossLive &e : live) {
    uint32_t a = 0, b = 0, r = 0;
    CHECK(p.problem_at(e.problem, &a, &b, &r));
    CHECK(a * R + r == e.row_a && b * R + r == e.row_b);
  }
  uint32_t a, b, r;
  CHECK(!p.problem_at((uint32_t)(p.tables->pairs() * R), &a, &b, &r));  // one past the last id
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
  const std::vector<NeedleHipSeq> rows = rows_of(len);
  CrossPairsShape sh;
  sh.residents = K;
  sh.arriving = N;
  sh.regions = R;
  sh.resident = rows.data();
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
  CHECK(p.labelled && p.problems() == p.live.size());
  check_cells_and_decode(p, p.live, len, K, N, R);

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
  std::vector<NeedleHipSeq> rows;
  for (size_t i = 0; len && i < K * R; i++) rows.push_back(NeedleHipSeq{0, len[i]});
  sh.resident = len ? rows.data() : nullptr;
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
  CHECK(says(error_of(2, 2, 1, lens.data(), nullptr, nullptr, nullptr), "null argument"));
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
  const std::vector<NeedleHipSeq> rows = rows_of(std::vector<uint32_t>(300, 2));
  sh.resident = rows.data();
  sh.resident_groups = res_groups.data();
  sh.groups = groups.data();
  sh.max_items = mi;
  const CrossPairsPlan p = plan_cross_pairs(sh);
  CHECK(p.error == nullptr && p.resident_pairs == 256 && p.arriving_pairs == 64 * 6 && p.live.size() == 640);
  CHECK(p.resident_hashes[0] == 64 * 2);  // only the 64 residents whose show arrives own hashes
}

// ---- the object without labels as it was planned before cross_pairs.h planned it: crossmatch.hip's own expressions ---------------
namespace before {

constexpr size_t kMaxLanes = 256;
constexpr size_t kMaxRegions = 2;
constexpr size_t kMaxProblems = 65535;
constexpr uint64_t kMaxRowItems = 0x7FFFFFF0ull;

const char *shape_error(const NeedleHipSeq *resident, size_t num_resident, size_t num_hashes, bool check_arena, size_t videos, size_t regions,
                        const size_t *max_items) {
  if (regions < 1 || regions > kMaxRegions) return "crossmatcher: regions must be 1 or 2";
  if (videos < (num_resident ? 1u : 2u) || videos > kMaxLanes)
    return num_resident ? "crossmatcher: arriving videos must be 1 to 256" : "crossmatcher: lanes (videos) must be 2 to 256";
  for (size_t r = 0; r < regions; r++)
    if (max_items[r] < 2 || max_items[r] > kMaxRowItems) return "crossmatcher: max_items must be 2 to 2^31 - 16";
  // (videos <= 256 and the first test bound num_resident before anything is multiplied)
  if (num_resident > kMaxProblems || (num_resident * videos + videos * (videos - 1) / 2) * regions > kMaxProblems)
    return "crossmatcher: more than 65 535 live problems ((K N + N (N - 1) / 2) x regions)";
  const uint64_t all = num_resident + videos;
  if (all * (all - 1) / 2 * regions >= (1ull << 32)) return "crossmatcher: the problem index over all videos does not fit 32 bits";
  for (size_t i = 0; i < num_resident * regions; i++) {
    if (resident[i].len > kMaxRowItems) return "crossmatcher: a resident row holds more than 2^31 - 16 hashes";
    if (check_arena && (uint64_t)resident[i].offset + resident[i].len > num_hashes) return "crossmatcher: a resident row lies outside the hash arena";
  }
  return nullptr;
}

// creation's checks in creation's order: the shape with the arena, then min_len
const char *creation_error(const NeedleHipSeq *resident, size_t num_resident, size_t num_hashes, size_t videos, size_t regions,
                           const size_t *max_items, const uint32_t *min_len) {
  if (const char *what = shape_error(resident, num_resident, num_hashes, true, videos, regions, max_items)) return what;
  for (size_t r = 0; r < regions; r++)
    if (min_len[r] == 0) return "crossmatcher: min_len must be >= 1";
  return nullptr;
}

size_t StateBytesResident(const NeedleHipSeq *resident, size_t num_resident, size_t videos, size_t regions, const size_t *max_items) {
  if (!max_items || (num_resident && !resident) || shape_error(resident, num_resident, 0, false, videos, regions, max_items)) return 0;
  bool narrow = true;
  for (size_t r = 0; r < regions; r++) narrow = narrow && max_items[r] < 65536;
  for (size_t i = 0; i < num_resident * regions; i++) narrow = narrow && resident[i].len < 65536;
  const size_t pairs = videos * (videos - 1) / 2, width = narrow ? sizeof(uint16_t) : sizeof(uint32_t);
  size_t bytes = 0;
  for (size_t r = 0; r < regions; r++) {
    size_t hashes = 0;  // S_r
    for (size_t k = 0; k < num_resident; k++) hashes += resident[k * regions + r].len;
    bytes += pairs * 2 * 2 * max_items[r] * width + videos * max_items[r] * sizeof(uint32_t)  // the arriving pairs' L frontiers, the histories
             + videos * 2 * hashes * width + hashes * sizeof(uint32_t);                        // the resident col frontiers, the resident hashes
  }
  return bytes;
}

struct CrossRegions {  // the fields of the kernels' argument that the layout fills
  uint64_t hist0, hist1, state0, state1, res_hist0, res_hist1, res_state0, res_state1, res_total0, res_total1;
};
struct CrossResident {
  uint64_t prefix;
  uint32_t len, src;
};
struct Layout {
  size_t videos = 0;
  bool narrow = true;
  CrossRegions rg{};
  uint64_t res_cell_rows[2] = {0, 0}, res_longest = 0;
  std::vector<CrossResident> table;
  size_t hist_words = 0, state_entries = 0, first_resident_word = 0;
  size_t pairs() const { return videos * (videos - 1) / 2; }
};

// the layout loop of creation
Layout layout(const NeedleHipSeq *resident, size_t num_resident, size_t videos, size_t regions, const size_t *max_items) {
  Layout m;
  m.videos = videos;
  std::vector<CrossResident> table(num_resident * regions);
  size_t res_total[2] = {0, 0};
  for (size_t k = 0; k < num_resident; k++)
    for (size_t r = 0; r < regions; r++) {
      const NeedleHipSeq &row = resident[k * regions + r];
      table[k * regions + r] = CrossResident{res_total[r], row.len, row.offset};
      res_total[r] += row.len;
      m.res_cell_rows[r] += std::max<uint64_t>(row.len, 1) - 1;
      m.res_longest = std::max<uint64_t>(m.res_longest, row.len);
      m.narrow = m.narrow && row.len < 65536;
    }
  size_t hist_words = 0, state_entries = 0;
  for (size_t r = 0; r < regions; r++) {
    m.narrow = m.narrow && max_items[r] < 65536;
    (r ? m.rg.hist1 : m.rg.hist0) = hist_words;
    (r ? m.rg.state1 : m.rg.state0) = state_entries;
    hist_words += videos * max_items[r];
    state_entries += m.pairs() * 4 * max_items[r];
  }
  const size_t first_resident_word = hist_words;
  for (size_t r = 0; r < regions; r++) {
    (r ? m.rg.res_hist1 : m.rg.res_hist0) = hist_words;
    (r ? m.rg.res_state1 : m.rg.res_state0) = state_entries;
    (r ? m.rg.res_total1 : m.rg.res_total0) = res_total[r];
    hist_words += res_total[r];
    state_entries += videos * 2 * res_total[r];
  }
  m.table.swap(table);
  m.hist_words = hist_words;
  m.state_entries = state_entries;
  m.first_resident_word = first_resident_word;
  return m;
}

}  // namespace before

static bool same_words(const char *x, const char *y) { return (!x && !y) || (x && y && std::strcmp(x, y) == 0); }

// One shape without labels: the plan's refusal is the old object's, word for word; where it is accepted, its layout is.
// Returns whether it was accepted.
static bool unlabelled_case(const std::vector<NeedleHipSeq> &rows, size_t K, size_t N, size_t R, const size_t *max_items, const uint32_t *min_len,
                            size_t arena) {
  CrossPairsShape sh;
  sh.residents = K;
  sh.arriving = N;
  sh.regions = R;
  sh.resident = rows.data();
  sh.max_items = max_items;
  sh.min_len = min_len;
  sh.arena_hashes = arena;
  const CrossPairsPlan p = plan_cross_pairs(sh);
  CHECK(same_words(p.error, before::creation_error(rows.data(), K, arena, N, R, max_items, min_len)));
  sh.min_len = nullptr;  // the question about sizes: no min_len, no arena
  sh.arena_hashes = ~0ull;
  const CrossPairsPlan sizes = plan_cross_pairs(sh);
  CHECK(same_words(sizes.error, before::shape_error(rows.data(), K, 0, false, N, R, max_items)));
  CHECK((sizes.error ? 0 : sizes.state_bytes()) == before::StateBytesResident(rows.data(), K, N, R, max_items));
  if (p.error) {
    CHECK(p.live.empty() && !p.state_entries && !p.hist_words && !p.tables);
    return false;
  }
  const before::Layout m = before::layout(rows.data(), K, N, R, max_items);
  CHECK(!p.labelled && p.labels.empty() && p.regions == R);
  CHECK(p.hist[0] == m.rg.hist0 && p.state[0] == m.rg.state0 && p.res_hist[0] == m.rg.res_hist0 && p.res_state[0] == m.rg.res_state0 &&
        p.resident_hashes[0] == m.rg.res_total0);
  if (R == 2)
    CHECK(p.hist[1] == m.rg.hist1 && p.state[1] == m.rg.state1 && p.res_hist[1] == m.rg.res_hist1 && p.res_state[1] == m.rg.res_state1 &&
          p.resident_hashes[1] == m.rg.res_total1);
  CHECK(p.hist_words == m.hist_words && p.state_entries == m.state_entries && p.res_hist[0] == m.first_resident_word);
  CHECK(p.narrow == m.narrow && p.longest_resident == m.res_longest);
  CHECK(p.state_bytes() == before::StateBytesResident(rows.data(), K, N, R, max_items));
  CHECK(p.problems() == (K * N + m.pairs()) * R);  // gridDim.y of the walk
  for (size_t i = 0; i < K * R; i++)  // the resident table as it is uploaded: every resident is live
    CHECK(p.resident_live[i / R] && p.resident_prefix[i] == m.table[i].prefix);
  CHECK(p.resident_cell_rows.size() == R && p.lane_group == std::vector<uint32_t>(N, 0u));
  for (size_t r = 0; r < R; r++) CHECK(p.resident_cell_rows[r] == m.res_cell_rows[r]);
  // the problems the closed form of the walk numbers, which the plan lists without being asked to
  CHECK(p.live.size() == p.problems());
  std::vector<uint32_t> len(K * R);
  for (size_t i = 0; i < K * R; i++) len[i] = rows[i].len;
  if (p.live.size() <= 4096) check_cells_and_decode(p, p.live, len, K, N, R);
  return true;
}

// every K <= 4, N <= 5, regions 1 and 2, rows of 0, 1 and more hashes, a capacity and a row on either side of the entry width,
// min_len with a zero, an arena that is too small
static size_t unlabelled_layouts() {
  size_t accepted = 0;
  static const uint32_t kLens[6] = {0u, 1u, 6u, 3u, 1u, 0u};
  for (size_t K = 0; K <= 4; K++)
    for (size_t N = 0; N <= 5; N++)
      for (size_t R = 1; R <= 2; R++)
        for (size_t variant = 0; variant < 12; variant++) {
          g_case = "unlabelled K=" + std::to_string(K) + " N=" + std::to_string(N) + " R=" + std::to_string(R) + " variant=" + std::to_string(variant);
          std::vector<uint32_t> len(K * R);
          for (size_t i = 0; i < len.size(); i++) len[i] = variant == 6 ? 0u : variant == 7 ? 1u : kLens[(i + variant) % 6];
          if (variant == 8 && !len.empty()) len.back() = 65536;   // one wide row
          if (variant == 9 && !len.empty()) len.front() = 65535;  // ... and the longest narrow one
          const size_t max_items[2] = {variant == 10 ? (size_t)65536 : 5, variant == 11 ? (size_t)65536 : 3};
          const std::vector<NeedleHipSeq> rows = rows_of(len);
          size_t arena = 0;
          for (uint32_t l : len) arena += l;
          static const uint32_t kMinLen[3][2] = {{1, 1}, {0, 1}, {3, 0}};
          for (size_t m = 0; m < 3; m++) accepted += unlabelled_case(rows, K, N, R, max_items, kMinLen[m], arena);
          if (arena) accepted += unlabelled_case(rows, K, N, R, max_items, kMinLen[0], arena - 1);
        }
  return accepted;
}

// the refusals, string for string, where a bound is met exactly and passed by one
static size_t unlabelled_boundaries() {
  size_t shapes = 0;
  static const size_t kK[8] = {0, 1, 255, 256, 32767, 32768, 65535, 65536}, kN[5] = {0, 1, 2, 256, 257};
  static const size_t kItems[6] = {1, 2, 65535, 65536, 0x7FFFFFF0, 0x7FFFFFF1};
  const uint32_t min_len[2] = {1, 1};
  std::vector<NeedleHipSeq> rows(2 * 65536, NeedleHipSeq{0, 2}), long_row = rows;
  for (size_t i = 0; i < long_row.size(); i += 255) long_row[i].len = 0x7FFFFFF1u;  // (row 0 of every shape among them)
  for (size_t K : kK)
    for (size_t N : kN)
      for (size_t R = 0; R <= 3; R++)
        for (size_t items : kItems)
          for (size_t which = 0; which < 2; which++) {
            g_case = "boundary K=" + std::to_string(K) + " N=" + std::to_string(N) + " R=" + std::to_string(R) + " max_items=" + std::to_string(items) +
                     (which ? " with a long row" : "");
            const size_t max_items[3] = {items, R == 2 && which ? 2 : items, items};
            (void)unlabelled_case(which ? long_row : rows, K, N, R, max_items, min_len, 2);
            shapes++;
          }
  return shapes;
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
  const size_t layouts = unlabelled_layouts(), boundaries = unlabelled_boundaries();
  std::printf("%zu cases\n%zu unlabelled layouts\n%zu boundary shapes\ncross pairs ok\n", cases, layouts, boundaries);
  return 0;
}
