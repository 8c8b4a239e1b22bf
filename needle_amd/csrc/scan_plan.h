// The all-pairs Hamming scan's launch plan, for the host and the device alike: the table entry the scan kernels read
// (SearchProblem), the geometry of the matrix-pipe form that decides what fits a workgroup, and build_plan(), which turns
// a list of sequence pairs into the table, the kernel choice and the grid.  Plain C++17, pure integer arithmetic: search.hip
// launches what it says, scan_mfma_kernel.h reads the table it packs, and tests/cpp/scan_plan_check.cpp runs these very
// functions on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "common.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEEDLE_HOST_DEVICE __host__ __device__
#else
#define NEEDLE_HOST_DEVICE
#endif

namespace needle {

constexpr int kDiagsPerBlock = 256;
constexpr int kBandR = 7, kBandU = 3;          // band kernel: 7 diagonals per lane, checkpoint every 21 rows
constexpr int kBandB = 64 * kBandR;
constexpr int kSampleW = 8;                     // sampled kernel: rows per aligned window
constexpr int kSampleHead = 3;                  // rows of a window evaluated before the first early-out

struct SearchProblem {
  uint32_t src_off, n;  // hash arena offset + length of the source sequence
  uint32_t dst_off, m;
  uint32_t min_len, tag;
  uint32_t block_base;  // first workgroup of this problem in the grid; matrix-pipe form with images: image_first_window()
  uint32_t pad;         // matrix-pipe form: the group fields below; 0 otherwise
};

// SearchProblem::pad under the matrix-pipe form.  A GROUP is up to kM2Members neighbours of the sorted table that share a
// destination and a minimum length: one workgroup's work (times the launch's split count).
//   bits 0 .. 7    of a group's first entry: how many followers stand behind it
//   bit 31         set on a follower (it owns no workgroups)
//   bits 8 .. 30   of the entry at POSITION G, whatever group that entry belongs to: the index of group G's first entry -- the
//                  table is its own directory, so a workgroup finds its group with one load
constexpr int kPadFollowersBits = 8, kPadDirectoryBits = 23;
constexpr uint32_t kPadFollowerFlag = 1u << 31;
constexpr size_t kPadDirectoryEntries = (size_t)1 << kPadDirectoryBits;   // staged entries one matrix-pipe launch can name
static_assert(kPadFollowersBits + kPadDirectoryBits == 31, "followers, directory and the follower flag fill the word");
NEEDLE_HOST_DEVICE constexpr uint32_t pad_first_entry(uint32_t followers) { return followers; }
NEEDLE_HOST_DEVICE constexpr uint32_t pad_directory_entry(uint32_t first) { return first << kPadFollowersBits; }   // OR-ed in
NEEDLE_HOST_DEVICE constexpr uint32_t pad_followers(uint32_t pad) { return pad & ((1u << kPadFollowersBits) - 1u); }
NEEDLE_HOST_DEVICE constexpr bool pad_is_follower(uint32_t pad) { return (pad & kPadFollowerFlag) != 0; }
NEEDLE_HOST_DEVICE constexpr uint32_t pad_directory(uint32_t pad) { return (pad >> kPadFollowersBits) & ((1u << kPadDirectoryBits) - 1u); }
// SearchProblem::block_base of a staged entry in a matrix-pipe launch with window images (that kernel finds its work through
// the directory and reads no workgroup number): the first window of the entry's source in the launch's images.
NEEDLE_HOST_DEVICE constexpr uint32_t image_first_window(const SearchProblem &p) { return p.block_base; }
inline void set_image_first_window(SearchProblem *p, uint32_t window) { p->block_base = window; }

NEEDLE_HOST_DEVICE constexpr int mfma_windows(int n, int min_len, int W) {
  return (n - 1 - W) >= 0 && min_len - W + 1 > 0 ? (n - 1 - W) / (min_len - W + 1) + 1 : 0;  // w0 = 1 + k P, w0 + W - 1 <= n - 1
}

// ---- geometry of the matrix-pipe form (scan_mfma_kernel.h tells what the pieces are for) ----------------------------------
constexpr int kM2Heads = 4;
#ifndef NEEDLE_M2_MEMBERS
#define NEEDLE_M2_MEMBERS 12
#endif
constexpr int kM2Members = NEEDLE_M2_MEMBERS; // sources a workgroup takes at most (of one destination; its share of the CU's LDS decides: nine 24-minute
                                              // windows, four 45-minute ones); < 16: a window's member rides in 4 bits.  (8 until round 6: the ninth -- room
                                              // made by a run buffer of 32 instead of 64 -- is 2.2 % at 39 060 pairs of 24-minute windows: one more pair per setup,
                                              // 98 instead of 94 % of the row tiles' rows in use)
constexpr int kM2Pitch = kM2Heads * 4 + 4;    // words of a window's row in the A image: 4 x 32 FP4 nibbles of +-1, the window's member << 28 | w0, 3 spare
                                              // (20: sixteen lanes' 16-byte reads of one instruction fall into sixteen different groups of four banks)
#ifndef NEEDLE_M2_RUNBUF
#define NEEDLE_M2_RUNBUF 32
#endif
constexpr int kM2RunBuf = NEEDLE_M2_RUNBUF;   // runs a workgroup collects in LDS before it asks for room in the run list (one atomic)
constexpr int kM2Table = 256;                 // a byte of hash bits -> its eight FP4 nibbles (bit set: +1 = 0x2, clear: -1 = 0xA)
constexpr int kM2Probe = 4;                   // rows looked at on either side of a whole window
constexpr int kM2Rows = kSampleW + 2 * kM2Probe;  // source hashes kept per window: its W rows and four probes on either side (m2_probe_offset)
constexpr int kM2ColBlocks = 2;               // column blocks of 32 positions a wave takes per unit
constexpr int kM2Queue = 128;                 // items a wave can hold: < 64 waiting + the <= 64 one turn adds
// The workgroup's control words (one table in LDS)
constexpr int kCtlUnits = 0;                              // units handed out
constexpr int kCtlRows = 1;                               // [+ g] first row (window) of member g; [+ members]: all rows
constexpr int kCtlSrc = kCtlRows + kM2Members + 1;        // [+ g] member g's source offset in the hash arena
constexpr int kCtlLen = kCtlSrc + kM2Members;             // [+ g] its length
constexpr int kCtlImage = kCtlLen + kM2Members;           // [+ g] first window of its image
constexpr int kCtlRuns = kCtlImage + kM2Members;          // runs collected in the workgroup's buffer
constexpr int kCtlSlot = kCtlRuns + 1;                    // their first slot in the run list
constexpr int kCtlTaken = kCtlSlot + 1;                   // chain queue: chains taken,
constexpr int kCtlPushed = kCtlTaken + 1;                 // chains pushed,
constexpr int kCtlLock = kCtlPushed + 1;                  // its lock
constexpr int kCtlThrough = kCtlLock + 1;                 // waves that have flushed their items
constexpr int kM2CtlWords = (kCtlThrough + 1 + 3) & ~3;   // (a multiple of 4: what follows stays 16-byte aligned)
#ifndef NEEDLE_M2_CHAINS
#define NEEDLE_M2_CHAINS 32
#endif
constexpr int kM2Chains = NEEDLE_M2_CHAINS;   // entries of the ring
static_assert((kM2Chains & (kM2Chains - 1)) == 0, "");

// LDS words of a workgroup: staged destination (+ 64 zeros), tables, per-window source hashes, A image
NEEDLE_HOST_DEVICE constexpr size_t m2_round4(size_t x) { return (x + 3) & ~(size_t)3; }
NEEDLE_HOST_DEVICE constexpr size_t m2_lds_words(uint64_t m, uint64_t windows, int waves) {
  return m2_round4(m + 64) + kM2CtlWords + kM2Table + 4 * kM2RunBuf + 2 * kM2Chains + (size_t)waves * kM2Queue + (size_t)(windows + 1) * (kM2Pitch + kM2Rows);
}

constexpr int kM2ImageWords = kM2Pitch + kM2Rows;   // per window
struct M2ImageSeq {
  uint32_t src_off, n;     // the sequence in the hash arena
  uint32_t first_window;   // of its image, in windows
  uint32_t windows;
};

static_assert(kM2Members - 1 <= (1 << kPadFollowersBits) - 1, "a group's followers fit their field of pad");

// ---- the plan ------------------------------------------------------------------------------------------------------------
// The switches that steer it: search.hip fills them from the threshold and the environment (scan_switches()), the planner
// reads nothing else.  EVERY switch the planner looks at is in here: the cached plan is keyed by them.
enum class MfmaRequest { Off, Forced, Automatic };   // the sampled scan's first stage on the matrix pipe
struct ScanSwitches {
  bool generic_only = false;        // NEEDLE_HIP_GENERIC_SEARCH: the one-lane-per-diagonal kernel whatever the minimum lengths
  bool band_only = false;           // NEEDLE_HIP_BAND_SEARCH: no sampled kernel
  int bands_per_wave = 0;           // NEEDLE_HIP_BANDS_PER_WAVE (tests, tuning); 0: by the size of the launch
  bool beyond_bit_trick = false;    // threshold > 31: every cell matches, the band / generic kernels take such a launch
  MfmaRequest mfma = MfmaRequest::Automatic;   // NEEDLE_HIP_SCAN_MFMA
  size_t lds_limit = 160 * 1024;    // LDS of a staged pair in bytes: the CU's, or NEEDLE_HIP_SEARCH_LDS_LIMIT (tests)
  int mfma_waves = 8;               // NEEDLE_HIP_MFMA_WAVES: the matrix-pipe form's waves per workgroup, 4 / 8 / 12 / 16
  int mfma_splits = 0;              // NEEDLE_HIP_MFMA_SPLITS (tests, tuning), 1 .. 64 workgroups per group; 0: by the number of groups
  bool mfma_single = false;         // NEEDLE_HIP_MFMA_SINGLE (tests, measurements): one source per workgroup
  bool mfma_no_images = false;      // NEEDLE_HIP_MFMA_NO_IMAGES: workgroups build their sources' windows themselves
  int window_w = kSampleW;          // rows per aligned window of the sampled scan (NEEDLE_HIP_SCAN_SHAPE)
  bool operator==(const ScanSwitches &o) const {
    return generic_only == o.generic_only && band_only == o.band_only && bands_per_wave == o.bands_per_wave &&
           beyond_bit_trick == o.beyond_bit_trick && mfma == o.mfma && lds_limit == o.lds_limit && mfma_waves == o.mfma_waves &&
           mfma_splits == o.mfma_splits && mfma_single == o.mfma_single && mfma_no_images == o.mfma_no_images && window_w == o.window_w;
  }
};

// What a launch needs besides its inputs: the device descriptors, the grid and the kernel choice.  Kept with the
// inputs it was derived from, so that a job that is run again (a library has ~n^2 / 2 pairs) rebuilds nothing.
struct SearchPlan {
  std::vector<NeedleHipSeq> seqs;          // inputs ...
  std::vector<NeedleHipProblem> problems;
  ScanSwitches switches;                   // ... and the switches that steered the choice
  std::vector<SearchProblem> meta;         // derived: the pairs the chosen kernel can stage, then the oversize ones
  size_t staged = 0;                       // how many of meta go to the chosen kernel
  uint64_t oversize_blocks = 0;            // grid of the unstaged kernel over meta[staged..]
  uint64_t blocks = 0;
  size_t lds_bytes = 0;
  bool sampled = false, fast = false, mfma = false;
  int mfma_waves = 0, mfma_splits = 1;      // scan_mfma_kernel.h: waves per workgroup, workgroups per group
  std::vector<M2ImageSeq> image_seqs;       // ... and the source sequences whose window images a pre-pass builds (empty: workgroups build their own)
  uint32_t image_windows = 0, image_min_len = 0;
  uint64_t mfma_products = 0;                 // v_mfma instructions a launch of the matrix-pipe form issues
  int bands_per_wave = 1;
  bool valid = false;
  bool matches(const NeedleHipSeq *s, size_t ns, const NeedleHipProblem *p, size_t np, const ScanSwitches &sw) const {
    return valid && seqs.size() == ns && problems.size() == np && switches == sw &&
           std::memcmp(seqs.data(), s, ns * sizeof(NeedleHipSeq)) == 0 &&
           std::memcmp(problems.data(), p, np * sizeof(NeedleHipProblem)) == 0;
  }
};

inline Status scan_too_large() { return Status::Make(NeedleError_InvalidArgument, "hamming_runs: too many problems for one launch"); }
inline uint64_t scan_windows(const SearchProblem &m) { return (uint64_t)mfma_windows((int)m.n, (int)m.min_len, kSampleW); }
inline uint64_t scan_diag_blocks(const SearchProblem &m) { return ((uint64_t)m.n + m.m - 3 + kDiagsPerBlock - 1) / kDiagsPerBlock; }
inline uint64_t scan_bands(const SearchProblem &m) { return ((uint64_t)m.n + m.m - 3 + kBandB - 1) / kBandB; }

// ---- groups of the matrix-pipe form ----------------------------------------------------------------------------------------
// A workgroup's LDS for a destination of m hashes and `windows` source windows, and what a group may take of it so that the
// intended number of workgroups share a CU (LDS comes in granules of 1280 bytes: 53 760 is a third of a CU's, 81 920 half).
inline size_t m2_group_bytes(uint32_t m, uint64_t windows, int waves) { return m2_lds_words(m, windows, waves) * sizeof(uint32_t); }
inline size_t m2_group_budget(int waves) { return waves == 4 ? 53760 : waves == 8 ? 81920 : 163840; }
// The matrix-pipe kernel packs its queue items as unit << 17 | batch of row tiles << 11 | lane << 5 | flag bit and a window /
// member word as w0 | member << 28 (scan_mfma_kernel.h): a group has fewer than 8192 windows, a staged entry m < 65536 and
// n < 2^28.  The 160 KiB of LDS imply the first two (m <= ~40 900) only while the limit is the hardware's; checked so that an
// overridden limit or a future layout cannot break the packing silently -- such an entry goes to the oversize partition.
constexpr uint64_t kM2GroupWindows = 8192;
inline bool m2_packable(const SearchProblem &m) { return m.m < 65536u && scan_windows(m) < kM2GroupWindows && m.n < (1u << 28); }

struct ScanGroup {
  size_t first, members;   // meta[first .. first + members)
  uint64_t windows;        // of all members: the rows of the group's tiles
};
// The ONE walk over a table sorted by destination: neighbours with the same destination, length and minimum form a group of
// up to kM2Members while the group's LDS stays within the budget.  Its two callers differ in two rules, on purpose:
//   single      every entry a group of its own (NEEDLE_HIP_MFMA_SINGLE).  The automatic choice's estimate never passes it: the
//               switch is for measurements of the forced form, and the choice is about the grouping a launch would get by itself.
//   window_cap  a group ends before kM2GroupWindows windows, the packing's limit.  The assignment keeps it; the estimate, which
//               also looks at entries that will turn out oversize, leaves it out as it always has.  Every budget there is ends
//               a group far earlier (build_plan's static_assert), so today the rule cuts nothing in either.
inline std::vector<ScanGroup> scan_groups(const SearchProblem *meta, size_t count, int waves, bool single, bool window_cap) {
  std::vector<ScanGroup> groups;
  const size_t budget = m2_group_budget(waves);
  for (size_t i = 0; i < count;) {
    const SearchProblem &a = meta[i];
    ScanGroup g{i, 1, scan_windows(a)};
    for (; !single && g.members < (size_t)kM2Members && i + g.members < count; g.members++) {
      const SearchProblem &b = meta[i + g.members];
      const uint64_t windows = g.windows + scan_windows(b);
      if (a.dst_off != b.dst_off || a.m != b.m || a.min_len != b.min_len || (window_cap && windows >= kM2GroupWindows) ||
          m2_group_bytes(a.m, windows, waves) > budget)
        break;
      g.windows = windows;
    }
    groups.push_back(g);
    i += g.members;
  }
  return groups;
}

// ---- build_plan's stages ---------------------------------------------------------------------------------------------------
// 1. The table from the problems.  A pair with a sequence of fewer than two hashes has no cell with i >= 1 and j >= 1
// (comparator.rs:165-167,179) and no entry.
inline Status scan_table(const NeedleHipSeq *seqs, size_t num_seqs, const NeedleHipProblem *problems, size_t num_problems,
                         std::vector<SearchProblem> *meta) {
  meta->clear();
  meta->reserve(num_problems);
  for (size_t p = 0; p < num_problems; p++) {
    const NeedleHipProblem &pr = problems[p];
    if (pr.src_seq >= num_seqs || pr.dst_seq >= num_seqs)
      return Status::Make(NeedleError_InvalidArgument, "hamming_runs: problem references a missing sequence");
    if (pr.min_len == 0) return Status::Make(NeedleError_InvalidArgument, "hamming_runs: min_len must be >= 1");
    const NeedleHipSeq &a = seqs[pr.src_seq], &b = seqs[pr.dst_seq];
    if (a.len < 2 || b.len < 2) continue;
    meta->push_back(SearchProblem{a.offset, a.len, b.offset, b.len, pr.min_len, pr.tag, 0u, 0u});
  }
  return Status::Ok();
}

// 2. Kernel choice.  The sampled kernel needs min_len >= 2 W - 1 + 8 of every problem, the band kernel its checkpoint spacing;
// otherwise (tiny minimum durations) the general one-lane-per-diagonal kernel handles the launch.
// The matrix-pipe form of the sampled scan pays on large launches whose windows fill their row tiles of 32 (sources of one
// destination share a workgroup's tiles): measured against the vector form, scan kernel, 1.41 x at 39 060 pairs of 24-minute
// windows (2 x 39 windows in 3 tiles), 1.66 x at 499 500 pairs of 45-minute ones (2 x 73 in 5); 0.97 x on the headline's 378
// pairs, where the scan hides beside the next job's first pass anyway.  From how many pairs: with FP4 products it is the faster
// kernel from ~2000 pairs of 24-minute windows up (0.127 against 0.142 ms at 2016, 0.19 / 0.33 at 4950, 0.26 / 0.62 at 9730,
// 0.38 / 0.83 at 16 110) and jobs are no slower with it from there on either (two in flight, the scan beside the next job's
// first pass: 1.56 / 1.56, 2.65 / 2.71, 4.08 / 4.12, 5.66 / 5.96 ms).  A candidate launch has its table SORTED by destination
// here (the runs carry the index of their own entry: its order is free) and keeps that order whatever the choice.
constexpr size_t kMfmaFromPairs = 2048;
inline void scan_choose_kernel(const ScanSwitches &sw, SearchPlan *plan) {
  std::vector<SearchProblem> &meta = plan->meta;
  uint32_t smallest = 0xFFFFFFFFu;
  for (const SearchProblem &m : meta) smallest = std::min(smallest, m.min_len);
  plan->sampled = !sw.generic_only && !sw.band_only && !sw.beyond_bit_trick && smallest >= (uint32_t)(2 * sw.window_w - 1 + 8);
  plan->fast = !sw.generic_only && !plan->sampled && smallest >= (uint32_t)(kBandR * kBandU);
  plan->mfma = plan->sampled && sw.mfma == MfmaRequest::Forced;
  if (!plan->mfma && !(plan->sampled && sw.mfma == MfmaRequest::Automatic && meta.size() >= kMfmaFromPairs)) return;
  std::stable_sort(meta.begin(), meta.end(), [](const SearchProblem &a, const SearchProblem &b) {
    if (a.dst_off != b.dst_off) return a.dst_off < b.dst_off;
    if (a.m != b.m) return a.m < b.m;
    return a.min_len < b.min_len;
  });
  if (plan->mfma) return;
  uint64_t windows = 0, rows = 0;  // automatic: where the windows of a group fill at least 70 % of its row tiles of 32
  for (const ScanGroup &g : scan_groups(meta.data(), meta.size(), sw.mfma_waves, false, false)) {
    windows += g.windows;
    rows += (g.windows + 31) / 32 * 32;
  }
  plan->mfma = rows > 0 && 10 * windows >= 7 * rows;
}

// What a pair needs in LDS under the chosen kernel (the matrix-pipe form: as a group of its own).
inline size_t scan_entry_bytes(const SearchPlan &plan, const ScanSwitches &sw, const SearchProblem &m) {
  if (plan.mfma) return m2_group_bytes(m.m, scan_windows(m), sw.mfma_waves);
  return ((plan.fast || plan.sampled) ? (size_t)m.m + 2 * kBandB : (size_t)m.n + m.m) * sizeof(uint32_t);
}

// 3. The partition.  A pair beyond the CU's 160 KiB (a window of more than ~2.7 h of audio at step 1), or one the matrix-pipe
// form cannot pack, goes to the end of the table and is scanned from HBM by the unstaged kernel, one workgroup per 256
// consecutive diagonals as in the generic staged form: one such video must not fail the search of the whole library (the
// reference has no bound).  Limit: the unstaged grid.
inline Status scan_partition(const ScanSwitches &sw, SearchPlan *plan) {
  std::vector<SearchProblem> &meta = plan->meta;
  auto stageable = [&](const SearchProblem &m) {
    return scan_entry_bytes(*plan, sw, m) <= sw.lds_limit && (!plan->mfma || m2_packable(m));
  };
  plan->staged = (size_t)(std::stable_partition(meta.begin(), meta.end(), stageable) - meta.begin());
  plan->oversize_blocks = 0;
  for (size_t i = plan->staged; i < meta.size(); i++) {
    meta[i].block_base = (uint32_t)plan->oversize_blocks;
    plan->oversize_blocks += scan_diag_blocks(meta[i]);
  }
  return plan->oversize_blocks > 0x7FFFFFFFull ? scan_too_large() : Status::Ok();
}

// 4. The grid for the chosen kernel.  Bands per wave of the sampled kernel: enough workgroups to fill the chip several times
// over with one band per wave; beyond that, more bands per wave so that each workgroup's staging of the destination sequence
// serves more of its pair.  (The band kernel has one whatever this says, the matrix-pipe form none; the plan carries the
// number all the same, as it always has.)
inline int scan_bands_per_wave(const ScanSwitches &sw, const SearchPlan &plan) {
  if (!plan.fast && !plan.sampled) return 1;
  if (sw.bands_per_wave > 0) return sw.bands_per_wave;
  uint64_t total_bands = 0;
  for (size_t i = 0; i < plan.staged; i++) total_bands += scan_bands(plan.meta[i]);
  int bands_per_wave = 1;
  while (plan.sampled && bands_per_wave < 8 && total_bands / (4 * (uint64_t)bands_per_wave * 2) >= 16384) bands_per_wave *= 2;
  return bands_per_wave;
}

// 4a. The generic, band and sampled kernels: an entry's workgroups follow those of the entry before it.  Limit: the grid.
inline Status scan_vector_grid(const ScanSwitches &sw, SearchPlan *plan) {
  const bool bands = plan->fast || plan->sampled;
  const uint64_t per_block = 4 * (uint64_t)(plan->sampled ? plan->bands_per_wave : 1);
  for (size_t i = 0; i < plan->staged; i++) {
    SearchProblem &m = plan->meta[i];
    m.block_base = (uint32_t)plan->blocks;
    plan->blocks += bands ? (scan_bands(m) + per_block - 1) / per_block : scan_diag_blocks(m);
    plan->lds_bytes = std::max(plan->lds_bytes, scan_entry_bytes(*plan, sw, m));
  }
  return plan->blocks > 0x7FFFFFFFull ? scan_too_large() : Status::Ok();
}

// 4b. The matrix-pipe form: the groups of the staged entries, their pad words and the directory; one workgroup per
// group, and a launch of few groups splits each over several (column units strided).  Limits: the directory's width, the grid.
inline Status scan_matrix_grid(const ScanSwitches &sw, int cus, SearchPlan *plan) {
  static_assert(m2_lds_words(0, kM2GroupWindows - 1, 4) * sizeof(uint32_t) > 163840, "every budget ends a group before the window cap");
  std::vector<SearchProblem> &meta = plan->meta;
  if (plan->staged >= kPadDirectoryEntries) return scan_too_large();
  const std::vector<ScanGroup> groups = scan_groups(meta.data(), plan->staged, sw.mfma_waves, sw.mfma_single, true);
  const uint64_t slots = (uint64_t)cus * (uint64_t)(sw.mfma_waves == 4 ? 3 : sw.mfma_waves == 8 ? 2 : 1);
  if (!groups.empty()) plan->mfma_splits = (int)std::min<uint64_t>(8, std::max<uint64_t>(1, (2 * slots + groups.size() - 1) / groups.size()));
  if (!groups.empty() && sw.mfma_splits > 0) plan->mfma_splits = sw.mfma_splits;
  for (size_t g = 0; g < groups.size(); g++) {
    const ScanGroup &grp = groups[g];
    SearchProblem *a = &meta[grp.first];
    for (size_t k = 0; k < grp.members; k++) {
      a[k].pad = k ? kPadFollowerFlag : pad_first_entry((uint32_t)(grp.members - 1));
      // (a follower's: where the next group begins.  This kernel reads neither -- see image_first_window())
      a[k].block_base = (uint32_t)((g + (k ? 1 : 0)) * (uint64_t)plan->mfma_splits);
    }
    meta[g].pad |= pad_directory_entry((uint32_t)grp.first);   // g <= grp.first: that entry's own fields are in place
    plan->lds_bytes = std::max(plan->lds_bytes, m2_group_bytes(a->m, grp.windows, sw.mfma_waves));
    if (grp.windows > 0 && a->m >= (uint32_t)kSampleW + 1) {
      uint64_t col_blocks = ((uint64_t)a->m - kSampleW) / 32 + 1;
      col_blocks = (col_blocks + kM2ColBlocks - 1) / kM2ColBlocks * kM2ColBlocks;  // whole units are multiplied
      plan->mfma_products += (grp.windows + 31) / 32 * col_blocks * (kM2Heads / 2);
    }
  }
  plan->blocks = groups.size() * (uint64_t)plan->mfma_splits;
  return plan->blocks > 0x7FFFFFFFull ? scan_too_large() : Status::Ok();
}

// 5. The matrix-pipe form's window images (scan_mfma_kernel.h): one per distinct source sequence, when the launch has ONE
// minimum length (a library of equal-length videos; otherwise the window positions differ per pair and workgroups build
// their own).  Limit: 2 GB of images -- beyond it, as with nothing to build, the workgroups build their own too.
inline void scan_images(const ScanSwitches &sw, SearchPlan *plan) {
  std::vector<SearchProblem> &meta = plan->meta;
  if (!plan->mfma || plan->staged == 0 || sw.mfma_no_images) return;
  for (size_t i = 1; i < plan->staged; i++)
    if (meta[i].min_len != meta[0].min_len) return;
  std::unordered_map<uint64_t, uint32_t> first_of;   // (src_off, n) -> first window
  uint64_t total = 0;
  for (size_t i = 0; i < plan->staged; i++) {
    const uint64_t key = ((uint64_t)meta[i].src_off << 32) | meta[i].n;
    auto it = first_of.find(key);
    if (it == first_of.end()) {
      const uint32_t w = (uint32_t)scan_windows(meta[i]);
      it = first_of.emplace(key, (uint32_t)total).first;
      plan->image_seqs.push_back(M2ImageSeq{meta[i].src_off, meta[i].n, (uint32_t)total, w});
      total += w;
    }
    set_image_first_window(&meta[i], it->second);
  }
  if (total == 0 || total * kM2ImageWords * sizeof(uint32_t) > ((uint64_t)1 << 31)) {
    plan->image_seqs.clear();
  } else {
    plan->image_windows = (uint32_t)total;
    plan->image_min_len = meta[0].min_len;
  }
}

// cus: the device's compute units (the matrix-pipe form's split count).
inline Status build_plan(const NeedleHipSeq *seqs, size_t num_seqs, const NeedleHipProblem *problems, size_t num_problems,
                         const ScanSwitches &sw, int cus, SearchPlan *plan) {
  plan->valid = plan->sampled = plan->fast = plan->mfma = false;
  plan->staged = plan->lds_bytes = 0;
  plan->blocks = plan->oversize_blocks = plan->mfma_products = 0;
  plan->image_seqs.clear();
  plan->image_windows = plan->image_min_len = 0;
  plan->mfma_waves = sw.mfma_waves;
  plan->mfma_splits = plan->bands_per_wave = 1;
  Status s = scan_table(seqs, num_seqs, problems, num_problems, &plan->meta);
  if (s.ok() && !plan->meta.empty()) {
    scan_choose_kernel(sw, plan);
    if ((s = scan_partition(sw, plan)).ok()) {
      plan->bands_per_wave = scan_bands_per_wave(sw, *plan);
      s = plan->mfma ? scan_matrix_grid(sw, cus, plan) : scan_vector_grid(sw, plan);
    }
    if (s.ok()) scan_images(sw, plan);
  }
  if (!s.ok()) return s;
  plan->seqs.assign(seqs, seqs + num_seqs);
  plan->problems.assign(problems, problems + num_problems);
  plan->switches = sw;
  plan->valid = true;
  return Status::Ok();
}

}  // namespace needle
