// Host-side check of needle_amd/csrc/scan_plan.h: the all-pairs scan's launch plan for synthetic tables that take every
// branch of the planner (tests/test_scan_plan_cpu.py lists them), 256 compute units.  For every case it asserts what the
// kernels rely on, independently of any recorded output; with --record it prints one line per case -- the plan's scalar
// fields and a 64-bit FNV-1a digest of its table and image list -- which the test compares with tests/golden/scan_plans.txt,
// recorded from the planner as it stood before it was taken apart into stages.  --time: the host time of one large plan.
// Lengths are in hashes; no hash is ever read, so the arenas the offsets point into do not exist.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../needle_amd/csrc/scan_plan.h"

using namespace needle;

namespace {

constexpr int kCus = 256;
constexpr MfmaRequest kOff = MfmaRequest::Off, kForced = MfmaRequest::Forced;
using Switches = ScanSwitches;

struct Table {
  std::vector<NeedleHipSeq> seqs;
  std::vector<NeedleHipProblem> problems;
  uint32_t add_seq(uint32_t len) {
    const uint32_t off = seqs.empty() ? 0u : seqs.back().offset + seqs.back().len;
    seqs.push_back(NeedleHipSeq{off, len});
    return (uint32_t)seqs.size() - 1;
  }
  void add(uint32_t src, uint32_t dst, uint32_t min_len) {
    problems.push_back(NeedleHipProblem{src, dst, min_len, (uint32_t)problems.size()});
  }
};

// the first `count` pairs (a, b), a < b, of `videos` sequences in the comparator's order; length of video v = len + v * ragged
Table pairs_of(uint32_t videos, size_t count, uint32_t len, uint32_t min_len, uint32_t ragged = 0) {
  Table t;
  for (uint32_t v = 0; v < videos; v++) t.add_seq(len + v * ragged);
  for (uint32_t a = 0; a < videos; a++)
    for (uint32_t b = a + 1; b < videos; b++)
      if (t.problems.size() < count) t.add(a, b, min_len);
  return t;
}
Table all_pairs(uint32_t videos, uint32_t len, uint32_t min_len) { return pairs_of(videos, (size_t)-1, len, min_len); }

// `sources` sequences against one destination
Table one_destination(uint32_t sources, uint32_t src_len, uint32_t dst_len, uint32_t min_len) {
  Table t;
  const uint32_t dst = t.add_seq(dst_len);
  for (uint32_t s = 0; s < sources; s++) t.add(t.add_seq(src_len), dst, min_len);
  return t;
}

Status plan_for(const Table &t, const Switches &sw, SearchPlan *plan) {
  return build_plan(t.seqs.data(), t.seqs.size(), t.problems.data(), t.problems.size(), sw, kCus, plan);
}

// the table's packing, through the decoders the matrix-pipe kernel uses
bool is_follower(const SearchProblem &m) { return pad_is_follower(m.pad); }
uint32_t followers(const SearchProblem &m) { return pad_followers(m.pad); }
uint32_t directory(const SearchProblem &m) { return pad_directory(m.pad); }

uint64_t windows_of(const SearchProblem &m) { return (uint64_t)mfma_windows((int)m.n, (int)m.min_len, kSampleW); }
uint64_t diag_blocks(const SearchProblem &m) { return ((uint64_t)m.n + m.m - 3 + kDiagsPerBlock - 1) / kDiagsPerBlock; }
size_t group_budget(int waves) { return waves == 4 ? 53760 : waves == 8 ? 81920 : 163840; }

int g_failed = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      std::printf("%s: INVARIANT ", name);                    \
      std::printf(__VA_ARGS__);                               \
      std::printf(" (%s)\n", #cond);                          \
      g_failed++;                                             \
      return;                                                 \
    }                                                         \
  } while (0)

// What the kernels rely on, for any plan.
void check_invariants(const char *name, const SearchPlan &p, const Switches &sw) {
  const std::vector<SearchProblem> &meta = p.meta;
  CHECK(p.staged <= meta.size(), "staged beyond the table");
  CHECK(!(p.mfma && !p.sampled) && !(p.sampled && p.fast), "one kernel");
  // every staged entry fits the chosen kernel's LDS under the limit (and the matrix-pipe form's packing)
  for (size_t i = 0; i < p.staged; i++) {
    const SearchProblem &m = meta[i];
    const size_t need = p.mfma ? m2_lds_words(m.m, windows_of(m), sw.mfma_waves) * 4
                               : ((p.sampled || p.fast) ? (size_t)m.m + 2 * kBandB : (size_t)m.n + m.m) * 4;
    CHECK(need <= sw.lds_limit && need <= p.lds_bytes, "entry %zu needs %zu bytes", i, need);
    if (p.mfma) CHECK(m.m < 65536u && windows_of(m) < 8192u && m.n < (1u << 28), "entry %zu cannot be packed", i);
  }
  CHECK(p.lds_bytes <= std::max(sw.lds_limit, p.mfma ? group_budget(sw.mfma_waves) : 0), "lds_bytes %zu", p.lds_bytes);
  // the oversize partition: 256 diagonals per workgroup
  uint64_t ob = 0;
  for (size_t i = p.staged; i < meta.size(); i++) {
    CHECK(meta[i].block_base == ob, "oversize entry %zu starts at %u, not %llu", i, meta[i].block_base, (unsigned long long)ob);
    ob += diag_blocks(meta[i]);
  }
  CHECK(ob == p.oversize_blocks, "oversize grid");
  CHECK(p.blocks <= 0x7FFFFFFFull && ob <= 0x7FFFFFFFull, "grid beyond 2^31");
  if (!p.mfma) {  // block_base: non-decreasing, the sum of the workgroups before; the grid is the sum of all
    uint64_t base = 0;
    for (size_t i = 0; i < p.staged; i++) {
      const SearchProblem &m = meta[i];
      CHECK(m.block_base == base, "entry %zu starts at %u, not %llu", i, m.block_base, (unsigned long long)base);
      CHECK(m.pad == 0, "pad of entry %zu", i);
      if (p.sampled || p.fast) {
        const uint64_t bands = ((uint64_t)m.n + m.m - 3 + kBandB - 1) / kBandB, per_block = 4 * (uint64_t)(p.sampled ? p.bands_per_wave : 1);
        base += (bands + per_block - 1) / per_block;
      } else {
        base += diag_blocks(m);
      }
    }
    CHECK(base == p.blocks, "grid %llu, entries sum to %llu", (unsigned long long)p.blocks, (unsigned long long)base);
    CHECK(p.image_seqs.empty() && p.image_windows == 0, "images without the matrix pipe");
    return;
  }
  // matrix-pipe form: groups of one destination; followers contiguous behind their first entry
  size_t groups = 0, max_need = 0;
  uint64_t products = 0;
  const bool images = !p.image_seqs.empty();
  // (block_base of a matrix-pipe entry is its first workgroup only where the planner never tried images: where it tried and
  // gave them up -- no windows at all, more than 2 GB -- the entries keep the windows it had numbered, which nothing reads)
  bool images_tried = !sw.mfma_no_images;
  for (size_t i = 1; i < p.staged; i++) images_tried = images_tried && meta[i].min_len == meta[0].min_len;
  for (size_t i = 0; i < p.staged;) {
    const SearchProblem &a = meta[i];
    CHECK(!is_follower(a), "entry %zu should begin a group", i);
    const uint32_t f = followers(a);
    CHECK(f + 1 <= (uint32_t)kM2Members && i + f < p.staged, "group at %zu has %u followers", i, f);
    uint64_t windows = windows_of(a);
    for (uint32_t k = 1; k <= f; k++) {
      const SearchProblem &b = meta[i + k];
      CHECK(is_follower(b) && followers(b) == 0, "entry %zu should follow %zu", i + k, i);
      CHECK(b.dst_off == a.dst_off && b.m == a.m && b.min_len == a.min_len, "entry %zu is of another group than %zu", i + k, i);
      windows += windows_of(b);
    }
    CHECK(i + f + 1 == p.staged || !is_follower(meta[i + f + 1]), "more followers behind %zu than its count %u", i, f);
    CHECK(!sw.mfma_single || f == 0, "a group in a launch of singles");
    const size_t need = m2_lds_words(a.m, windows, sw.mfma_waves) * 4;
    CHECK(windows < 8192 && (f == 0 || need <= group_budget(sw.mfma_waves)), "group at %zu: %llu windows, %zu bytes", i,
          (unsigned long long)windows, need);
    max_need = std::max(max_need, need);
    // entry G of the table names group G's first entry
    CHECK(directory(meta[groups]) == i, "directory entry %zu names %u, not %zu", groups, directory(meta[groups]), i);
    if (!images_tried)
      for (uint32_t k = 0; k <= f; k++)  // (a follower: where the next group begins)
        CHECK(meta[i + k].block_base == (groups + (k ? 1 : 0)) * (uint64_t)p.mfma_splits, "entry %zu: first workgroup %u", i + k, meta[i + k].block_base);
    if (windows > 0 && a.m >= (uint32_t)kSampleW + 1) {
      const uint64_t col_blocks = (((uint64_t)a.m - kSampleW) / 32 + 1 + kM2ColBlocks - 1) / kM2ColBlocks * kM2ColBlocks;
      products += (windows + 31) / 32 * col_blocks * (kM2Heads / 2);
    }
    groups++;
    i += f + 1;
  }
  for (size_t g = groups; g < p.staged; g++) CHECK(directory(meta[g]) == 0, "directory entry %zu beyond the groups", g);
  CHECK(p.staged < kPadDirectoryEntries, "directory too narrow for %zu entries", p.staged);
  CHECK(p.blocks == groups * (uint64_t)p.mfma_splits, "grid %llu of %zu groups x %d", (unsigned long long)p.blocks, groups, p.mfma_splits);
  CHECK(p.mfma_splits >= 1 && p.mfma_splits <= 64 && p.mfma_waves == sw.mfma_waves, "splits, waves");
  CHECK(p.lds_bytes == max_need, "lds_bytes %zu, largest group %zu", p.lds_bytes, max_need);
  CHECK(p.mfma_products == products, "products");
  // images: one per distinct source, each entry's window = its source's first one, image_windows = their sum
  if (images) {
    CHECK(!sw.mfma_no_images, "images in a launch without");
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> first;
    uint64_t total = 0;
    for (const M2ImageSeq &q : p.image_seqs) {
      CHECK(q.first_window == total, "image of %u starts at %u", q.src_off, q.first_window);
      CHECK(first.emplace(std::make_pair(q.src_off, q.n), q.first_window).second, "two images of one source");
      CHECK(q.windows == (uint32_t)mfma_windows((int)q.n, (int)p.image_min_len, kSampleW), "windows of an image");
      total += q.windows;
    }
    CHECK(total == p.image_windows && total * kM2ImageWords * 4 <= ((uint64_t)1 << 31), "image_windows");
    for (size_t i = 0; i < p.staged; i++) {
      auto it = first.find(std::make_pair(meta[i].src_off, meta[i].n));
      CHECK(it != first.end() && image_first_window(meta[i]) == it->second && meta[i].min_len == p.image_min_len, "entry %zu: image window", i);
    }
  } else {
    CHECK(p.image_windows == 0, "image_windows without images");
  }
}

uint64_t fnv1a(uint64_t h, const void *data, size_t bytes) {
  const unsigned char *b = (const unsigned char *)data;
  for (size_t i = 0; i < bytes; i++) h = (h ^ b[i]) * 0x100000001B3ull;
  return h;
}

// The automatic choice's estimate, restated: groups of one destination up to kM2Members and the LDS budget, over the whole
// sorted table; how full their row tiles of 32 are.
double fill_ratio(const Table &t, int waves) {
  std::map<std::pair<uint32_t, uint32_t>, std::vector<uint64_t>> by_dst;  // (destination, min_len) -> windows of its sources
  for (const NeedleHipProblem &p : t.problems)
    by_dst[{p.dst_seq, p.min_len}].push_back((uint64_t)mfma_windows((int)t.seqs[p.src_seq].len, (int)p.min_len, kSampleW));
  uint64_t windows = 0, rows = 0;
  for (const auto &d : by_dst) {
    const uint64_t m = t.seqs[d.first.first].len;
    for (size_t i = 0; i < d.second.size();) {
      uint64_t w = d.second[i++];
      for (int k = 1; k < kM2Members && i < d.second.size() && m2_lds_words(m, w + d.second[i], waves) * 4 <= group_budget(waves); k++)
        w += d.second[i++];
      windows += w;
      rows += (w + 31) / 32 * 32;
    }
  }
  return rows ? (double)windows / (double)rows : 0.0;
}

bool g_record = false;

// One case: plan, invariants, one line.  `want`: the branch the case is there for ("" = only recorded).
void run_case(const char *name, const Table &t, const Switches &sw, const std::string &want = "", const char *note = nullptr) {
  SearchPlan p;
  const Status s = plan_for(t, sw, &p);
  if (!s.ok()) {
    if (want != "error") std::printf("%s: WANTED %s, got an error\n", name, want.c_str()), g_failed++;
    if (g_record) std::printf("%s error=\"%s\"\n", name, s.message.c_str());
    return;
  }
  check_invariants(name, p, sw);
  const char *form = p.staged == 0 ? "none" : p.mfma ? "matrix" : p.sampled ? "sampled" : p.fast ? "band" : "generic";
  if (!want.empty() && want != form) std::printf("%s: WANTED %s, got %s\n", name, want.c_str(), form), g_failed++;
  size_t groups = 0, largest = 0;
  for (size_t i = 0; i < p.staged && p.mfma; i++)
    if (!is_follower(p.meta[i])) groups++, largest = std::max<size_t>(largest, followers(p.meta[i]) + 1);
  if (!g_record) return;
  uint64_t h = 0xCBF29CE484222325ull;
  h = fnv1a(h, p.meta.data(), p.meta.size() * sizeof(SearchProblem));
  h = fnv1a(h, p.image_seqs.data(), p.image_seqs.size() * sizeof(M2ImageSeq));
  std::printf("%s form=%s entries=%zu staged=%zu oversize=%zu blocks=%llu oversize_blocks=%llu lds_bytes=%zu sampled=%d fast=%d mfma=%d "
              "mfma_waves=%d mfma_splits=%d bands_per_wave=%d mfma_products=%llu groups=%zu largest_group=%zu images=%zu image_windows=%u "
              "image_min_len=%u%s%s digest=%016llx\n",
              name, form, p.meta.size(), p.staged, p.meta.size() - p.staged, (unsigned long long)p.blocks,
              (unsigned long long)p.oversize_blocks, p.lds_bytes, (int)p.sampled, (int)p.fast, (int)p.mfma, p.mfma ? p.mfma_waves : 0,
              p.mfma_splits, p.bands_per_wave, (unsigned long long)p.mfma_products, groups, largest, p.image_seqs.size(), p.image_windows,
              p.image_min_len, note ? " " : "", note ? note : "", (unsigned long long)h);
}

// a library episode's opening half at 0.3 s a hash: 24 minutes -> 2400 hashes, a 20 s minimum -> 67
constexpr uint32_t kLen24 = 2400, kMin20s = 67;

void kernel_choice() {
  Switches sw;
  for (uint32_t min_len : {20u, 21u, 22u, 23u}) {
    const std::string name = "choice_min_len_" + std::to_string(min_len);
    run_case(name.c_str(), all_pairs(3, 300, min_len), sw, min_len < 21 ? "generic" : min_len < 23 ? "band" : "sampled");
  }
  Table mixed = all_pairs(4, 300, 40);  // the smallest minimum of a launch decides
  mixed.problems[3].min_len = 22;
  run_case("choice_smallest_of_mixed", mixed, sw, "band");
  Switches beyond = sw;
  beyond.beyond_bit_trick = true;  // threshold 32
  beyond.mfma = kOff;
  run_case("choice_beyond_bit_trick", all_pairs(3, 300, 23), beyond, "band");
  Switches band = sw;
  band.band_only = true;
  run_case("choice_band_only", all_pairs(3, 300, 23), band, "band");
  Switches generic = sw;
  generic.generic_only = true;
  run_case("choice_generic_only", all_pairs(3, 300, 23), generic, "generic");
  Switches wide = sw;  // a window of 16 rows: sampled from 2 * 16 - 1 + 8 = 39
  wide.window_w = 16;
  wide.mfma = kOff;
  run_case("choice_window16_min_len_38", all_pairs(3, 300, 38), wide, "band");
  run_case("choice_window16_min_len_39", all_pairs(3, 300, 39), wide, "sampled");
}

void automatic() {
  Switches sw;
  run_case("auto_2047_pairs", pairs_of(65, 2047, kLen24, kMin20s), sw, "sampled");
  run_case("auto_2048_pairs", pairs_of(65, 2048, kLen24, kMin20s), sw, "matrix");
  Switches off = sw;
  off.mfma = kOff;
  run_case("auto_2048_pairs_switched_off", pairs_of(65, 2048, kLen24, kMin20s), off, "sampled");
  // 2080 pairs whose groups fill their row tiles badly: 40 destinations so long that the LDS budget leaves room for ONE source's
  // windows beside them, 52 sources of 33 .. 45 windows (one tile of 32 and a few rows of the next)
  Table ragged;
  for (uint32_t d = 0; d < 40; d++) ragged.add_seq(16600 + 4 * d);
  for (uint32_t s = 0; s < 52; s++) ragged.add_seq(9 + 60 * (32 + s % 13) + 7 * s % 60);
  for (uint32_t d = 0; d < 40; d++)
    for (uint32_t s = 0; s < 52; s++) ragged.add(40 + s, d, kMin20s);
  const double full = fill_ratio(pairs_of(65, 2048, kLen24, kMin20s), sw.mfma_waves), poor = fill_ratio(ragged, sw.mfma_waves);
  if (!(full >= 0.7 && poor < 0.7)) std::printf("auto: fill ratios %.4f and %.4f do not straddle 0.7\n", full, poor), g_failed++;
  char note[64];
  std::snprintf(note, sizeof note, "fill=%.4f", poor);
  run_case("auto_2080_ragged_pairs", ragged, sw, "sampled", note);
  std::snprintf(note, sizeof note, "fill=%.4f", full);
  run_case("auto_2080_pairs", pairs_of(65, 2080, kLen24, kMin20s), sw, "matrix", note);
}

void forced() {
  Switches sw;
  sw.mfma = kForced;
  for (int waves : {4, 8, 12, 16}) {
    Switches w = sw;
    w.mfma_waves = waves;
    run_case(("forced_waves_" + std::to_string(waves)).c_str(), all_pairs(30, kLen24, kMin20s), w, "matrix");
    // fourteen sources of 100 windows and a destination of 6000: the LDS budget cuts the groups (1, 3 and 9 sources)
    run_case(("forced_lds_budget_waves_" + std::to_string(waves)).c_str(), one_destination(14, 6000, 6000, kMin20s), w, "matrix");
  }
  for (int splits : {1, 64}) {
    Switches s = sw;
    s.mfma_splits = splits;
    run_case(("forced_splits_" + std::to_string(splits)).c_str(), all_pairs(30, kLen24, kMin20s), s, "matrix");
  }
  run_case("forced_few_groups_split_8", all_pairs(4, kLen24, kMin20s), sw, "matrix");
  run_case("forced_many_groups", all_pairs(120, 600, kMin20s), sw, "matrix");
  Switches single = sw;
  single.mfma_single = true;
  run_case("forced_single", all_pairs(30, kLen24, kMin20s), single, "matrix");
  Switches plain = sw;
  plain.mfma_no_images = true;
  run_case("forced_no_images", all_pairs(30, kLen24, kMin20s), plain, "matrix");
  Table two = all_pairs(30, kLen24, kMin20s);  // two minimum lengths in one launch: no images, groups per minimum
  for (size_t i = 0; i < two.problems.size(); i += 2) two.problems[i].min_len = 82;
  run_case("forced_two_min_len", two, sw, "matrix");
  run_case("forced_members_plus_3", one_destination(kM2Members + 3, 600, 600, kMin20s), sw, "matrix");
  // The cap of 8192 windows per group: every LDS budget ends a group long before (8191 windows are 1.1 MB of images), so the
  // longest group there can be -- sources of one window -- is cut by the member count and the largest of windows by the budget
  static_assert(m2_lds_words(0, 8191, 4) * 4 > 163840, "the window cap is implied by the budgets");
  Switches w16 = sw;
  w16.mfma_waves = 16;
  run_case("forced_most_windows_per_group", one_destination(6, 16009, 100, 23), w16, "matrix");
  run_case("forced_no_windows", all_pairs(5, 8, 23), sw, "matrix");  // sequences too short for one window
  run_case("forced_short_destination", one_destination(3, 600, 8, 23), sw, "matrix");
}

void oversize() {
  // nine videos, the last three long: the limit keeps destinations of 1000 and sends those of 3000 to the unstaged kernel
  Table t;
  for (uint32_t v = 0; v < 9; v++) t.add_seq(v < 6 ? 1000 : 3000);
  for (uint32_t a = 0; a < 9; a++)
    for (uint32_t b = a + 1; b < 9; b++) t.add(a, b, kMin20s);
  Switches vec;
  vec.mfma = kOff;
  vec.lds_limit = (2000 + 2 * kBandB) * 4;
  run_case("oversize_third_sampled", t, vec, "sampled");
  Switches mat = vec;
  mat.mfma = kForced;
  mat.lds_limit = 20000;
  run_case("oversize_third_matrix", t, mat, "matrix");
  Switches generic = vec;
  generic.generic_only = true;
  generic.lds_limit = 2500 * 4;
  run_case("oversize_generic", t, generic, "generic");
  Switches all = vec;
  all.lds_limit = 1;
  run_case("oversize_everything", t, all, "none");
  // a destination of 70 000 hashes under a raised limit: within the limit, beyond the matrix-pipe form's 16-bit column
  Table wide = all_pairs(6, kLen24, kMin20s);
  const uint32_t big = wide.add_seq(70000);
  wide.add(0, big, kMin20s);
  wide.add(big, 1, kMin20s);
  Switches raised;
  raised.mfma = kForced;
  raised.lds_limit = 1 << 20;
  run_case("oversize_unpackable_matrix", wide, raised, "matrix");
}

void images() {
  Switches sw;
  sw.mfma = kForced;
  Table t;  // one source against fifty destinations: one image
  const uint32_t src = t.add_seq(kLen24);
  for (uint32_t d = 0; d < 50; d++) t.add(src, t.add_seq(kLen24), kMin20s);
  run_case("images_one_source", t, sw, "matrix");
  // more than 2 GB of images, from lengths alone: 15 000 sources of 1000 windows (36 words a window)
  Table huge;
  for (uint32_t s = 0; s < 15000; s++) huge.add_seq(9 + 16 * 999);
  const uint32_t dst = huge.add_seq(100);
  for (uint32_t s = 0; s < 15000; s++) huge.add(s, dst, 23);
  Switches w16 = sw;
  w16.mfma_waves = 16;
  run_case("images_beyond_2gb", huge, w16, "matrix");
  huge.problems.resize(14000);
  run_case("images_below_2gb", huge, w16, "matrix");
}

void bands_per_wave() {
  Switches sw;
  sw.mfma = kOff;  // pairs of 20 000 hashes: 90 bands each
  for (uint32_t videos : {54u, 55u, 78u, 109u})
    run_case(("bands_per_wave_" + std::to_string(videos) + "_videos").c_str(), all_pairs(videos, 20000, kMin20s), sw, "sampled");
  Switches three = sw;
  three.bands_per_wave = 3;
  run_case("bands_per_wave_override", all_pairs(109, 20000, kMin20s), three, "sampled");
  Switches band = three;
  band.band_only = true;  // the band kernel has one band per wave whatever the switch says
  run_case("bands_per_wave_band_kernel", all_pairs(109, 20000, kMin20s), band, "band");
}

void edges() {
  Switches sw;
  run_case("edge_no_problems", Table(), sw, "none");
  Table tiny = all_pairs(4, 300, 23);  // sequences of 0 and 1 hashes: their pairs have no cell
  const uint32_t zero = tiny.add_seq(0), one = tiny.add_seq(1);
  tiny.add(0, zero, 23);
  tiny.add(one, 1, 23);
  tiny.add(zero, one, 23);
  run_case("edge_lengths_0_and_1", tiny, sw, "sampled");
  Table only_tiny;
  only_tiny.add(only_tiny.add_seq(1), only_tiny.add_seq(500), 23);
  run_case("edge_nothing_but_skipped", only_tiny, sw, "none");
  Table missing = all_pairs(3, 300, 23);
  missing.add(0, 3, 23);
  run_case("edge_missing_sequence", missing, sw, "error");
  Table zero_min = all_pairs(3, 300, 23);
  zero_min.problems[1].min_len = 0;
  run_case("edge_min_len_0", zero_min, sw, "error");
  // 2^23 entries of the smallest pair there is: one more than the table's directory field can name
  Table many;
  many.add_seq(2);
  many.problems.assign((size_t)1 << 23, NeedleHipProblem{0, 0, 23, 0});
  Switches forced = sw;
  forced.mfma = kForced;
  run_case("edge_directory_full", many, forced, "error");
}

int time_plans() {  // 1000 videos of 45 minutes, all pairs: what a plan costs the host
  const Table t = all_pairs(1000, 4500, kMin20s);
  Switches sw;
  std::vector<double> ms;
  for (int r = 0; r < 9; r++) {
    SearchPlan p;
    const auto t0 = std::chrono::steady_clock::now();
    if (!plan_for(t, sw, &p).ok() || !p.mfma || p.staged != t.problems.size()) return std::printf("FAILED\n"), 1;
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  std::printf("plan of %zu pairs: median %.2f ms, min %.2f, max %.2f (9 plans)\n", t.problems.size(), ms[4], ms[0], ms[8]);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--time")) return time_plans();
  g_record = argc > 1 && !std::strcmp(argv[1], "--record");
  kernel_choice();
  automatic();
  forced();
  oversize();
  images();
  bands_per_wave();
  edges();
  std::printf("%s\n", g_failed ? "FAILED" : "scan plans ok");
  return g_failed ? 1 : 0;
}
