// What the ranks of a library job (library.cpp: needle_hip_library_job_begin / _end) send each other, decided on the
// host in plain C++17 -- no HIP, no getenv -- so that it can be checked without a device or a second process
// (tests/cpp/job_plan_check.cpp).  plan_job() decides the form of the epilogue, how the runs travel, every size and every
// offset a collective is given; judge() decides from the counts that came down whether the job is done or what has to grow
// before its scan is repeated.  Both are pure: every rank calls them with the same history and the same counts and must
// arrive at the same plan and the same verdict, or the ranks wait for each other in different collectives.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "common.h"
#include "shard.h"

namespace needle {

// ---- layout of a run slab and of the count matrix: the one place that knows it
// A slab (a rank's run list, a gathered head, a block of the directed exchange): 32-byte header, word 0 = runs found --
// which may exceed what the slab holds -- then the runs.
constexpr size_t kSlabHeader = 32;
inline size_t slab_bytes(uint32_t runs) { return kSlabHeader + (size_t)runs * sizeof(NeedleHipRun); }
// The count matrix: one row of count_words(world) words per rank, [runs in its slab, runs directed to rank 0, 1, ...],
// padded to a multiple of four words (an all-gather's block).
inline size_t count_words(int world) { return ((size_t)world + 1 + 3) & ~(size_t)3; }
inline size_t count_matrix_bytes(int world) { return count_words(world) * (size_t)world * sizeof(uint32_t); }
inline uint32_t slab_count(const uint32_t *matrix, int world, size_t r) { return matrix[r * count_words(world)]; }
inline uint32_t directed_count(const uint32_t *matrix, int world, size_t r, size_t q) { return matrix[r * count_words(world) + 1 + q]; }

// run capacities are multiples of 4 below 2^32 (a count that would round beyond stays at the largest of them)
inline uint32_t round_up4(uint64_t v) { return (uint32_t)std::min<uint64_t>((v + 3) & ~(uint64_t)3, 0xfffffffcu); }
// the next job's head or block after a job that needed `count` runs: an eighth more plus 64
inline uint32_t with_head_margin(uint32_t count) { return round_up4((uint64_t)count + count / 8 + 64); }
// the slab after one that overflowed at `count` runs: a quarter more plus 64
inline uint32_t with_slab_margin(uint32_t count) { return round_up4((uint64_t)count + count / 4 + 64); }

// (= pair_count of needle_core.h, which is not a header-only function)
inline uint64_t job_pairs(size_t n) { return n < 2 ? 0 : (uint64_t)n * (n - 1) / 2; }

// ---- inputs
// An environment hook of the job path as library.cpp's job_switches() found it: atoi of its value when set.
struct JobHook {
  bool set = false;
  int value = 0;
};
// Read at every job_begin, at every repeat and at every job_end: tests change them between the jobs of one process.
struct JobSwitches {
  JobHook device_epilogue;       // NEEDLE_HIP_DEVICE_EPILOGUE: 1 / 0 forces the form
  JobHook shard_epilogue;        // NEEDLE_HIP_SHARD_EPILOGUE: 1 / 0 forces each rank to its own block of videos
  JobHook shard_epilogue_pairs;  // NEEDLE_HIP_SHARD_EPILOGUE_PAIRS: the sharding threshold (tests)
  JobHook directed_runs;         // NEEDLE_HIP_DIRECTED_RUNS: 0 = every job travels as heads (measurements, tests)
  JobHook head_runs;             // NEEDLE_HIP_HEAD_RUNS: a library's first head (tests: one that overflows)
  JobHook slab_runs;             // NEEDLE_HIP_SLAB_RUNS: a library's first slab (tests: one that overflows)
  JobHook test_directed_cap;     // NEEDLE_HIP_TEST_DIRECTED_CAP: the first sized exchange gets blocks of this size, once
  JobHook test_epilogue_fail_rank;  // NEEDLE_HIP_TEST_EPILOGUE_FAIL_RANK: the device form "fails" on that rank alone
};

// What a library remembers of its last finished job (every rank remembers the same).
struct JobHistory {
  uint32_t slab_runs = 0;            // per-rank run capacity of the next job (grows on overflow); 0: no job yet
  uint32_t last_max_count = 0;       // largest per-rank run count: sizes the one-trip download
  std::vector<uint32_t> dir_counts;  // [world][world]: runs rank r directed to rank q (the block sizes' source)
  int dir_world = 0;
  bool dir_unsupported = false;      // the communicator has no point-to-point transfers: every job travels as heads
  bool dir_cap_forced = false;       // NEEDLE_HIP_TEST_DIRECTED_CAP was applied once
};

struct JobShape {
  size_t n = 0;                   // videos
  size_t arena_regions = 1;       // rows per video in the library's arena
  size_t comparator_regions = 1;  // NeedleHipRun.problem = pair * comparator_regions + region
  int world = 1, rank = 0;
  // The job's pairs where they are not all pairs of the n videos: a library with groups of videos (pair_ids.h) searches
  // the pairs inside its groups only, in the grouped numbering.  kAllPairs: job_pairs(n).
  static constexpr uint64_t kAllPairs = ~(uint64_t)0;
  uint64_t pairs = kAllPairs;
  uint64_t pair_total() const { return pairs == kAllPairs ? job_pairs(n) : pairs; }
};

// ---- the plan
// The owner-directed exchange: a run of pair (i, j) travels to the owners of videos i and j only.
struct DirectedPlan {
  bool wanted = false;  // this job sorts its runs by destination and counts them (the count matrix is gathered)
  bool sized = false;   // ... and the last job's matrix gives block sizes: the runs travel owner-directed (else: as heads)
  bool refused = false;       // blocks beyond 4 GiB: the job fails on every rank
  bool cap_consumed = false;  // the forced test cap was used: the caller sets JobHistory::dir_cap_forced
  std::vector<uint32_t> cap;  // [world][world] runs: the block rank r sends to rank q (wanted; all 0 while not sized)
  // this rank's send side (= the kernels' DirectPlan: offset, capacity) and receive side, bytes
  std::vector<uint32_t> send_capacity;
  std::vector<size_t> send_off, send_bytes, recv_off, recv_bytes;
  size_t send_total = 0, recv_total = 0;
  size_t max_block_bytes = 0;  // the largest block any rank sends: the same number everywhere
};

// How the device epilogue reads the run list: one segment per rank.
enum class SegmentKind { Slab, Heads, Blocks };  // this rank's slab (one rank) / the gathered heads / the blocks received
struct SegmentLayout {
  SegmentKind kind = SegmentKind::Slab;
  uint32_t capacity = 0;              // of every segment, or 0 where they differ:
  std::vector<uint32_t> capacities;   // Blocks: per source rank
  uint64_t max_runs = 0;              // the sum of the capacities (sizes the workspaces)
};

struct JobPlan {
  JobShape shape;
  size_t pair_first = 0, pair_count = 0;    // this rank's range of the pair ids (lexicographic, or grouped)
  size_t video_first = 0, video_count = 0;  // the videos whose results this rank computes (all of them unless sharded)
  // the form of the epilogue
  bool device_epilogue = false;  // on the device, enqueued behind the gather (else on host threads in job_end)
  bool sharded = false;          // each rank for its own block of videos + one gather of result blocks
  bool shape_fixed = false;      // `sharded` stands whatever job_end finds (else job_end decides it by the run count)
  bool inject_epilogue_failure = false;  // tests: this rank reports the device form as failed after enqueueing it
  uint32_t slab_runs = 0, head_runs = 0;
  size_t pinned_bytes = 0;  // what the one-trip download of the heads needs
  DirectedPlan directed;
  SegmentLayout segments;  // as the runs are planned to travel (segment_layout(plan, false) after the "unsupported" fallback)
  size_t head_bytes() const { return slab_bytes(head_runs); }
};

inline SegmentLayout segment_layout(const JobPlan &p, bool directed) {
  SegmentLayout s;
  const size_t W = (size_t)p.shape.world;
  if (directed) {  // the blocks received: one segment per source rank, each of its own capacity
    s.kind = SegmentKind::Blocks;
    for (size_t r = 0; r < W; r++) {
      s.capacities.push_back(p.directed.cap[r * W + (size_t)p.shape.rank]);
      s.max_runs += s.capacities.back();
    }
    return s;
  }
  s.kind = p.shape.world > 1 ? SegmentKind::Heads : SegmentKind::Slab;
  s.capacity = p.shape.world > 1 ? p.head_runs : p.slab_runs;
  s.max_runs = (uint64_t)s.capacity * (uint64_t)p.shape.world;
  return s;
}

// The per-video epilogue on the device (epilogue.hip) instead of on host threads: at library scale, where the host form
// takes tens of milliseconds and every rank of a node has only its share of the CPUs.  Decided when the job is enqueued
// (the run count is not known yet): by the number of sequence pairs, or by what the library's last finished job found --
// content decides the run count: 28 episodes with stretches of silence give their 378 pairs 41 528 runs instead of 852,
// and the host form 2.5 ms of a 0.5 ms job.  (Every rank sees every rank's count: the same decision everywhere.)
inline bool device_epilogue_wanted(const JobShape &sh, const JobSwitches &sw, const JobHistory &h) {
  if (sw.device_epilogue.set) return sw.device_epilogue.value != 0;
  return sh.pair_total() * sh.comparator_regions >= kDeviceEpiloguePairs || h.last_max_count >= kDeviceEpilogueRuns;
}

// The sizes: the slab of a library's first job, and the one-trip download -- everything the last job needed plus a
// margin, the whole slab while all slabs together are at most 1 MiB.
inline void plan_sizes(const JobSwitches &sw, const JobHistory &h, uint32_t keep_head, JobPlan *p) {
  const JobShape &sh = p->shape;
  p->slab_runs = h.slab_runs;
  if (p->slab_runs == 0 && sw.slab_runs.set) p->slab_runs = round_up4((uint64_t)std::max(4, sw.slab_runs.value));
  if (p->slab_runs == 0)
    p->slab_runs = round_up4(std::max<uint64_t>(1024, 4 * (uint64_t)shard_block((size_t)sh.pair_total(), sh.world) * sh.arena_regions));
  uint32_t head = h.last_max_count ? with_head_margin(h.last_max_count) : 4096u;
  const bool forced = !h.last_max_count && sw.head_runs.set;  // a first head only
  if (forced) head = round_up4((uint64_t)std::max(4, sw.head_runs.value));
  head = std::min(head, p->slab_runs);
  if (!forced && slab_bytes(p->slab_runs) * (size_t)sh.world <= (1u << 20)) head = p->slab_runs;
  p->head_runs = keep_head ? keep_head : head;
  p->pinned_bytes = p->head_bytes() * (size_t)sh.world;
}

// The epilogue's form (the exchange depends on it): on the device or on host threads, every rank for all videos or --
// more than one rank and a library large enough to pay for one more collective -- each for its own block (the decision
// cannot wait for the run count: the pairs stand in for it).
inline void plan_form(const JobSwitches &sw, const JobHistory &h, JobPlan *p) {
  const JobShape &sh = p->shape;
  p->device_epilogue = device_epilogue_wanted(sh, sw, h) && sh.n >= 2 && sh.pair_total() > 0;  // (no pair: the host form)
  // A rank whose device epilogue then fails alone keeps `sharded`: the other ranks enter the collective that decision implies.
  p->shape_fixed = p->device_epilogue;
  p->sharded = false;
  if (p->device_epilogue) {
    uint64_t shard_from = 1u << 16;
    if (sw.shard_epilogue_pairs.set) shard_from = (uint64_t)std::max(1, sw.shard_epilogue_pairs.value);
    p->sharded = sh.world > 1 && (sw.shard_epilogue.set ? sw.shard_epilogue.value != 0 : sh.pair_total() * sh.comparator_regions >= shard_from);
  }
  p->inject_epilogue_failure = p->device_epilogue && sw.test_epilogue_fail_rank.set && sw.test_epilogue_fail_rank.value == sh.rank;
  p->video_first = 0;
  p->video_count = sh.n;
  if (p->sharded) shard_range(sh.n, sh.world, sh.rank, &p->video_first, &p->video_count);
}

// Owner-directed exchange: with the sharded device epilogue a rank needs the runs of its own videos' pairs only.  Block
// sizes are host values on every rank: cap[r * world + q] comes from the count matrix of the library's last finished job
// plus a margin; a library's first job has no matrix yet: it counts, and travels as heads.  Worlds above 64 get no
// directed exchange (the kernels' DirectPlan has 64 entries).
inline void plan_directed(const JobSwitches &sw, const JobHistory &h, JobPlan *p) {
  const JobShape &sh = p->shape;
  DirectedPlan &d = p->directed;
  d = DirectedPlan();
  d.wanted = sh.world > 1 && sh.world <= 64 && p->device_epilogue && p->sharded && !h.dir_unsupported &&
             !(sw.directed_runs.set && sw.directed_runs.value == 0);
  if (!d.wanted) return;
  const size_t W = (size_t)sh.world, rank = (size_t)sh.rank;
  d.sized = h.dir_world == sh.world && h.dir_counts.size() == W * W;  // (a matrix of another world size sizes nothing)
  d.cap.assign(W * W, 0u);
  if (d.sized)
    for (size_t k = 0; k < W * W; k++) d.cap[k] = with_head_margin(h.dir_counts[k]);
  if (sw.test_directed_cap.set && d.sized && !h.dir_cap_forced) {  // tests: the library's first directed job gets blocks that overflow
    std::fill(d.cap.begin(), d.cap.end(), round_up4((uint64_t)std::max(4, sw.test_directed_cap.value)));
    d.cap_consumed = true;
  }
  d.send_capacity.resize(W);
  d.send_off.resize(W);
  d.send_bytes.resize(W);
  for (size_t q = 0; q < W; q++) {  // (not sized: headers only -- the send side still counts)
    d.send_capacity[q] = d.cap[rank * W + q];
    d.send_off[q] = d.send_total;
    d.send_bytes[q] = slab_bytes(d.send_capacity[q]);
    d.send_total += d.send_bytes[q];
  }
  for (size_t k = 0; k < W * W; k++) d.max_block_bytes = std::max(d.max_block_bytes, slab_bytes(d.cap[k]));
  d.refused = d.send_total >= 0xFFFFFFF0ull;  // the kernels' offsets are 32-bit
  d.recv_off.assign(W, 0);
  d.recv_bytes.assign(W, 0);
  if (d.sized)
    for (size_t r = 0; r < W; r++) {
      d.recv_off[r] = d.recv_total;
      d.recv_bytes[r] = slab_bytes(d.cap[r * W + rank]);
      d.recv_total += d.recv_bytes[r];
    }
}

// The whole plan of one attempt of a job.  On a repeat it is made AGAIN from the history judge() left, so the form can
// change between a job's first attempt and its repeat (last_max_count moved); every rank makes the same change.
// `keep_head` (JobVerdict): the one thing a repeat after a block overflow does not size again.
inline JobPlan plan_job(const JobShape &shape, const JobSwitches &sw, const JobHistory &h, uint32_t keep_head = 0) {
  JobPlan p;
  p.shape = shape;
  shard_range((size_t)shape.pair_total(), shape.world, shape.rank, &p.pair_first, &p.pair_count);
  plan_sizes(sw, h, keep_head, &p);
  plan_form(sw, h, &p);
  plan_directed(sw, h, &p);
  p.segments = segment_layout(p, p.directed.sized);
  return p;
}

// job_end, a job whose form was not fixed when it was enqueued (host epilogue): sharding the per-video epilogue costs one
// more (small) collective; it pays once the epilogue is milliseconds.  (`shard_epilogue`: NEEDLE_HIP_SHARD_EPILOGUE as job_end finds it.)
inline bool sharded_at_end(const JobPlan &p, const JobHook &shard_epilogue, size_t total_runs) {
  if (p.shape_fixed) return p.sharded;
  if (p.shape.world <= 1) return false;
  if (shard_epilogue.set) return shard_epilogue.value != 0;
  return total_runs >= (1u << 17);
}

// ---- the verdict
// What came down: every rank's slab count, and the count matrix when the job counted (wanted).  `directed`: the runs
// travelled owner-directed (planned as sized and the transport supports it).
struct JobCounts {
  bool directed = false;
  std::vector<uint32_t> slab;      // [world] runs each rank found (may exceed slab_runs)
  std::vector<uint32_t> directed_to;  // [world][world] runs rank r directed to rank q; empty: the job did not count
};
inline JobCounts counts_from_matrix(const uint32_t *matrix, int world, bool directed) {
  JobCounts c;
  c.directed = directed;
  for (size_t r = 0; r < (size_t)world; r++) {
    c.slab.push_back(slab_count(matrix, world, r));
    for (size_t q = 0; q < (size_t)world; q++) c.directed_to.push_back(directed_count(matrix, world, r, q));
  }
  return c;
}

enum class JobNext { Done, GrowHead, GrowBlocks, GrowSlab };
struct JobVerdict {
  JobNext next = JobNext::Done;
  uint32_t most = 0;   // the largest slab count
  uint32_t keep_head = 0;  // GrowBlocks: the repeat keeps this attempt's head (it travels directed and gathers none; should its
                           // form change at the repeat and that head be too short, the next verdict is GrowHead)
  JobHistory history;  // as the library must remember it from here on
};

// Every rank sees the same counts, so every rank draws the same verdict.  Anything but Done: the job's scan and exchange
// are repeated under a new plan made from `history` -- also after GrowBlocks, although the slab is intact.
inline JobVerdict judge(const JobPlan &p, const JobCounts &c, const JobHistory &before) {
  JobVerdict v;
  v.history = before;
  for (uint32_t n : c.slab) v.most = std::max(v.most, n);
  v.history.last_max_count = v.most;
  auto take_matrix = [&]() {  // the job's count matrix becomes the next job's block sizes
    v.history.dir_counts = c.directed_to;
    v.history.dir_world = p.shape.world;
  };
  if (v.most > p.slab_runs) {
    // some rank found more runs than a slab holds: the slab grows -- and the matrix, counted over a clamped slab, goes
    v.next = JobNext::GrowSlab;
    v.history.slab_runs = with_slab_margin(v.most);
    v.history.dir_counts.clear();
    return v;
  }
  if (c.directed) {  // a block that overflowed: the sizes follow the matrix just taken
    bool fits = true;
    for (size_t k = 0; k < c.directed_to.size() && fits; k++) fits = c.directed_to[k] <= p.directed.cap[k];
    take_matrix();
    v.next = fits ? JobNext::Done : JobNext::GrowBlocks;
    if (!fits) v.keep_head = p.head_runs;
    return v;
  }
  if (p.shape.world > 1 && v.most > p.head_runs) {  // some rank's list is longer than the head that was gathered
    v.next = JobNext::GrowHead;                      // (head_runs follows last_max_count; the matrix is not taken)
    return v;
  }
  if (!c.directed_to.empty()) take_matrix();  // a job that travelled as heads and counted: the next one can be directed
  return v;
}

}  // namespace needle
