// Streaming all-pairs comparator (include/needle_hip.h needle_hip_crossmatcher_*): N lanes whose hashes arrive in chunks,
// matched against each other.  Pair (a, b), a < b, is the problem (src = lane a, dst = lane b): both of its sides grow, and
// after any feeds its runs are those of needle_hip_hamming_runs_host over what the two lanes hold, reported as cells break them.
//
// State of a pair: the L-shaped frontier of its evaluated rectangle [0, Ja) x [0, Jb) -- col[i] = length of the matching
// diagonal stretch that ends at cell (i, Jb - 1), row[j] the same at cell (Ja - 1, j) for j < Jb - 1 (the corner is col's).
// u16 where max_items < 65 536, else u32; two sets of each.  Per lane, its hashes so far.
//
// One round (a feed, or a piece of one of at most kMaxStrip items per lane; also `finish`, with no items) is three launches
// -- crossmatch_land_kernel, crossmatch_walk_kernel, crossmatch_simhash_kernel -- whatever N and whichever lanes have data.
// The walk is stream_walk.h's, twice per pair: the column direction (X = lane a's rows, Y = lane b's new columns, from col)
// and its transpose for lane a's new rows (from row[j], j < Jb - 1).  col of (a, b) flips to its other set when lane b has
// items, row when lane a has; a side that only gains entries (the other lane grew) appends them to its current set.
// Nothing per pair is uploaded: a workgroup finds its pair from blockIdx.y, the lanes' progress in the round's lane table
// and the pair's state by arithmetic; the workgroups of a pair neither of whose lanes has data leave after reading two
// table entries.
//
// Regions (needle_hip_crossmatcher_new_regions): the lanes are videos x R, lane = video * R + region (R = 1 or 2: openings
// and endings, the numbering of the library's arena rows and of comparator.cpp's seqs), and only lanes of one region are
// matched against each other, each region with a capacity and a min_len of its own.  blockIdx.y of the walk is live pair * R
// + region; a region's max_items, min_len and bases travel by value in the kernels' arguments (CrossRegions).  Still three
// launches, one upload and one download per round; R = 1 is the same code with the second region's fields unused.
//
// Resident videos (needle_hip_crossmatcher_new_resident): K videos that are complete at creation come before the N arriving
// ones in the video list, V = K + N.  Only the arriving videos have lanes; a resident row (k, r) is a row of the resident
// table (CrossResident: its length and the sum of the lengths before it in its region, uploaded once), and the live problems
// are (a, b, r) with b >= K.  A resident is a lane that holds all its items, finished before the first round, with no new items
// ever: only the column direction has cells, and its state is the col frontier alone.  A resident is a complete X
// (stream_walk.h): a run that reaches its last row leaves with the round's runs, and the host holds it back until the arriving
// lane finishes, which is when the reporting rule hands out what is open on a frontier.
//
// Groups of videos (needle_hip_crossmatcher_new_grouped): every resident and every arriving video carries a label, and the live
// problems are the same-label pairs with an arriving end only.  State and hashes exist for live pairs only; the land and the
// simhash kernel do not know about groups: the rows travel in the run.
//
// Which problems are live, their order, NeedleHipRun.problem, where the hashes and every problem's state lie, what is
// allocated and every refusal are decided once for all these objects, on the host, by plan_cross_pairs (cross_pairs.h, which
// describes the layout); Create below executes that plan.  The walk takes its pair lookup as a policy: ClosedFormPairs (an
// object without labels: the plan's one-label layout by arithmetic, nothing uploaded) or ListedLivePairs (one entry of the
// plan's live-pair table, uploaded once next to the resident table, at an address the workgroup shares).
#include "crossmatch.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "stream_round.h"
#include "stream_walk.h"

namespace needle {

namespace {

constexpr uint32_t kParity = 1u;     // lane flags: the set that holds the state this lane's feeds flip
constexpr uint32_t kFinished = 2u;   // finished before this round
constexpr uint32_t kFinishing = 4u;  // finished by this round

struct CrossLane {
  uint32_t fed, width;  // J and the new items [J, J + width)
  uint32_t stage_off;   // of the new hashes inside the round's buffer, in words
  uint32_t flags;
};
static_assert(sizeof(CrossLane) == 16, "lane table entries are 4 words");

// What the kernels know of the regions, by value: nothing per region is uploaded in a round.  Named fields and selects,
// not arrays: an array indexed at run time can end up in scratch.
struct CrossRegions {
  uint32_t regions;                  // 1 or 2
  uint32_t max_items0, max_items1;   // capacity of a lane
  uint32_t min_len0, min_len1;
  uint64_t hist0, hist1;             // first word of the region's histories: row `video` is max_items words
  uint64_t state0, state1;           // first entry of the region's frontiers: pair p's four sets are 4 * max_items entries
  // resident videos: rows k * regions + r of the resident table
  uint32_t residents;                // K; 0: none of the fields below is read
  uint64_t res_hist0, res_hist1;     // first word of the region's resident hashes: row (k, r) starts `prefix` words on
  uint64_t res_state0, res_state1;   // first entry of the region's resident frontiers: (t, k) at 2 * (t * res_total + prefix)
  uint64_t res_total0, res_total1;   // S_r: the region's resident hashes
};

// One resident row, uploaded once at creation.
struct CrossResident {
  uint64_t prefix;  // the lengths of the region's rows before this one
  uint32_t len;
  uint32_t src;     // where the row lies in the arena it was taken from (crossmatch_gather_resident_kernel; no round reads it)
};
static_assert(sizeof(CrossResident) == 16, "resident table entries are 4 words");

__device__ __forceinline__ uint32_t region_max_items(const CrossRegions &rg, uint32_t r) { return r ? rg.max_items1 : rg.max_items0; }

// the history row of lane `lane` = video * regions + region
__device__ __forceinline__ uint64_t lane_row(const CrossRegions &rg, uint32_t lane) {
  const uint32_t r = rg.regions == 2u ? lane & 1u : 0u, video = rg.regions == 2u ? lane >> 1 : lane;
  return (r ? rg.hist1 : rg.hist0) + (uint64_t)video * region_max_items(rg, r);
}

// the hashes of row `row` = video * regions + region over all V videos: a resident's through the table, an arriving one's
// by arithmetic
__device__ __forceinline__ uint64_t video_row(const CrossRegions &rg, const CrossResident *__restrict__ resident, uint32_t row) {
  const uint32_t first = rg.residents * rg.regions;
  if (row >= first) return lane_row(rg, row - first);
  const uint32_t r = rg.regions == 2u ? row & 1u : 0u;
  return (r ? rg.res_hist1 : rg.res_hist0) + resident[row].prefix;
}

__global__ __launch_bounds__(kThreads) void crossmatch_land_kernel(const uint32_t *__restrict__ round_buf, uint32_t *__restrict__ hist,
                                                                   CrossRegions rg, uint32_t *__restrict__ count) {
  land_chunks<CrossLane>(round_buf, count, [&](const CrossLane &) { return hist + lane_row(rg, blockIdx.y); });
}

// Resident rows from an arena in device memory (the index store's) to where Create packs them: a workgroup per row,
// consecutive lanes move consecutive words.  Creation checked every row against the arena (plan_cross_pairs).
__global__ __launch_bounds__(kThreads) void crossmatch_gather_resident_kernel(const uint32_t *__restrict__ arena,
                                                                              const CrossResident *__restrict__ resident, uint32_t rows,
                                                                              CrossRegions rg, uint32_t *__restrict__ hist) {
  for (uint32_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const CrossResident rr = resident[row];
    const uint32_t r = rg.regions == 2u ? row & 1u : 0u;
    const uint32_t *__restrict__ from = arena + rr.src;
    uint32_t *__restrict__ to = hist + (r ? rg.res_hist1 : rg.res_hist0) + rr.prefix;
    for (uint32_t k = threadIdx.x; k < rr.len; k += kThreads) to[k] = from[k];
  }
}

// How crossmatch_walk_kernel finds its live problem blockIdx.y = q * regions + r: the two videos (of all V), whether the source
// is a resident, NeedleHipRun.problem and the first entry of the problem's state.  Built in the kernel from its arguments and
// its trailing ones (none for the closed form: its code is what it was), the way epilogue_kernels.h's pair policies are.
struct ClosedFormPairs {  // every pair with an arriving end: q = t * K + k for resident k against arriving video t, then the
  uint32_t a, b, pair;    // arriving pairs i-major as the comparator numbers them (pair_at in comparator.cpp): row ta holds
  bool res, live;         // videos - 1 - ta pairs
  __device__ ClosedFormPairs(const CrossRegions &rg, const uint32_t videos, const uint32_t q, const uint32_t) : pair(0u), live(true) {
    const uint32_t K = rg.residents;
    res = q < K * videos;
    if (res) {
      const uint32_t t = q / K;
      a = q - t * K;
      b = K + t;
    } else {
      pair = q - K * videos;
      uint32_t ta = 0u, first = 0u;
      while (pair - first >= videos - 1u - ta) {
        first += videos - 1u - ta;
        ta++;
      }
      a = K + ta;
      b = a + 1u + (pair - first);
    }
  }
  // the comparator's problem over V videos: row a of its pair numbering starts at a (2 V - a - 1) / 2
  __device__ uint32_t problem(const CrossRegions &rg, const uint32_t V, const uint32_t r) const {
    return (uint32_t)((uint64_t)a * (2u * V - a - 1u) / 2u + (b - a - 1u)) * rg.regions + r;
  }
  // an arriving pair's four sets by its number; a resident one's two at 2 * (t * S_r + prefix)
  __device__ uint64_t state_at(const CrossRegions &rg, const uint32_t r, const uint64_t prefix, const uint32_t max_items) const {
    return res ? (r ? rg.res_state1 : rg.res_state0) + 2u * ((uint64_t)(b - rg.residents) * (r ? rg.res_total1 : rg.res_total0) + prefix)
               : (r ? rg.state1 : rg.state0) + (uint64_t)pair * 4u * max_items;
  }
};
struct ListedLivePairs {  // the same-label pairs of a grouped object: one entry of the live-pair table (cross_pairs.h), at an address
  CrossLive e;        // every lane of the workgroup shares
  uint32_t a, b;
  bool res, live;
  __device__ ListedLivePairs(const CrossRegions &rg, const uint32_t, const uint32_t, const uint32_t problem_index,
                         const CrossLive *__restrict__ table, const uint32_t count)
      : live(problem_index < count) {  // (a labelling without live pairs still launches one row of workgroups)
    e = live ? table[problem_index] : CrossLive{};
    a = rg.regions == 2u ? e.row_a >> 1 : e.row_a;
    b = rg.regions == 2u ? e.row_b >> 1 : e.row_b;
    res = a < rg.residents;
  }
  __device__ uint32_t problem(const CrossRegions &, const uint32_t, const uint32_t) const { return e.problem; }
  __device__ uint64_t state_at(const CrossRegions &, const uint32_t, const uint64_t, const uint32_t) const { return e.state; }
};

template <typename T, class Pairs, class... Extra>
__global__ __launch_bounds__(kThreads) void crossmatch_walk_kernel(const uint32_t *__restrict__ hist, T *__restrict__ state,
                                                                   const CrossLane *__restrict__ lanes,
                                                                   const CrossResident *__restrict__ resident, uint32_t videos,
                                                                   CrossRegions rg, uint32_t side_blocks, uint32_t threshold,
                                                                   NeedleHipRun *__restrict__ runs, uint32_t capacity,
                                                                   uint32_t *__restrict__ count, Extra... extra) {
  __shared__ uint32_t strip[kMaxStrip];                // Y's new items
  __shared__ uint32_t rows[kCarriedRows + kMaxStrip];  // the X items this workgroup's diagonals meet
  // the live problem of this workgroup: q * regions + region, its videos by the policy
  const uint32_t per_side = side_blocks + kTopBlocks;
  const bool col_dir = blockIdx.x < per_side;
  const bool two = rg.regions == 2u;
  const uint32_t q = two ? blockIdx.y >> 1 : blockIdx.y, r = two ? blockIdx.y & 1u : 0u;
  const uint32_t K = rg.residents, V = K + videos, first_lane = two ? 2u * K : K;
  const Pairs lp(rg, videos, q, blockIdx.y, extra...);
  if (!lp.live) return;
  const bool res = lp.res;
  if (res && !col_dir) return;  // a resident gains no rows
  const uint32_t a = lp.a, b = lp.b;  // videos of all V
  const uint32_t problem = lp.problem(rg, V, r);
  const uint32_t row_a = two ? 2u * a + r : a, row_b = two ? 2u * b + r : b;
  const CrossLane lb = lanes[row_b - first_lane];
  // a resident is a lane that holds all its items, finished long ago
  CrossLane la;
  uint64_t prefix = 0u;
  if (res) {
    const CrossResident rr = resident[row_a];
    la = CrossLane{rr.len, 0u, 0u, kFinished};
    prefix = rr.prefix;
  } else {
    la = lanes[row_a - first_lane];
  }
  const uint32_t done_a = la.flags & (kFinished | kFinishing), done_b = lb.flags & (kFinished | kFinishing);
  const bool emit_open = done_a && done_b && ((la.flags | lb.flags) & kFinishing);  // the problem becomes complete in this round
  if (la.width == 0u && lb.width == 0u && !emit_open) return;                       // no state traffic
  const uint32_t a0 = max(la.fed, 1u), a1 = max(la.fed + la.width, 1u), b0 = max(lb.fed, 1u), b1 = max(lb.fed + lb.width, 1u);
  if (a1 < 2u || b1 < 2u) return;  // no cells yet: whatever the sets hold is not read before it is written
  const uint32_t max_items = region_max_items(rg, r), min_len = r ? rg.min_len1 : rg.min_len0;
  // an arriving pair: col set 0, row set 0, col set 1, row set 1, each of max_items; a resident one: col set 0, col set 1,
  // each of the row's own length
  const uint64_t at = lp.state_at(rg, r, prefix, max_items);
  const uint64_t col_stride = res ? (uint64_t)la.fed : 2u * (uint64_t)max_items;
  T *base = state + at;
  const uint32_t cs = lb.flags & kParity, rs = la.flags & kParity;
  const T *col_from = base + cs * col_stride, *row_from = base + (uint64_t)(2u * rs + 1u) * max_items;
  T *col_to = base + (cs ^ (lb.width ? 1u : 0u)) * col_stride;
  T *row_to = base + (uint64_t)(2u * (rs ^ (la.width ? 1u : 0u)) + 1u) * max_items;  // (no resident reads or writes a row set)
  const uint32_t *hb = hist + (r ? rg.hist1 : rg.hist0) + (uint64_t)(b - K) * max_items;
  const uint32_t *ha = res ? hist + (r ? rg.res_hist1 : rg.res_hist0) + prefix : hist + (r ? rg.hist1 : rg.hist0) + (uint64_t)(a - K) * max_items;
  const bool old_cells = a0 >= 2u && b0 >= 2u;
  // The two rows (video * regions + region over all videos, residents first) travel in the simhash fields until the simhash
  // kernel fills them.
  const auto sink = [&](const uint32_t src_end, const uint32_t dst_end, const uint32_t len) {
    return NeedleHipRun{problem, src_end, dst_end, len, row_a, row_b};
  };
  if (col_dir) {  // a resident row is a complete X: its carried diagonals end one entry earlier
    const WalkSide<T> sd{ha, hb, a1, b0, b1, res ? a0 - 1u : a0, old_cells ? col_from : nullptr, col_to, row_to, res};
    stream_walk<T, true>(strip, rows, sd, blockIdx.x, side_blocks, emit_open, threshold, min_len, runs, capacity, count, sink);
  } else {
    const WalkSide<T> sd{hb, ha, b1, a0, a1, b0 - 1u, old_cells ? row_from : nullptr, row_to, col_to, false};
    stream_walk<T, false>(strip, rows, sd, blockIdx.x - per_side, side_blocks, emit_open, threshold, min_len, runs, capacity, count, sink);
  }
}

__global__ __launch_bounds__(kThreads) void crossmatch_simhash_kernel(const uint32_t *__restrict__ hist,
                                                                      const CrossResident *__restrict__ resident, CrossRegions rg,
                                                                      NeedleHipRun *__restrict__ runs, uint32_t capacity,
                                                                      const uint32_t *__restrict__ count) {
  // src_match_hash, dst_match_hash come in as the two rows, video * regions + region over all videos
  simhash_runs(
      runs, capacity, count, [&](const NeedleHipRun &r) { return hist + video_row(rg, resident, r.src_match_hash); },
      [&](const NeedleHipRun &r) { return hist + video_row(rg, resident, r.dst_match_hash); });
}

struct LaneState {
  uint64_t fed = 0;
  bool finished = false;
  uint32_t parity = 0;
};

struct Piece {
  const uint32_t *items = nullptr;
  uint32_t width = 0;
  bool finishing = false;
};

}  // namespace

struct CrossMatcher::Impl {
  size_t n = 0, videos = 0, regions = 1;  // n = videos * regions lanes; lane = video * regions + region
  size_t max_items[2] = {0, 0};
  uint32_t min_len[2] = {0, 0}, threshold = 0;
  // what creation executed (cross_pairs.h): the layout, the pair tables, the labels, the entry width; its live-pair table is
  // kept, and was uploaded, for a labelled object only
  CrossPairsPlan plan;
  CrossRegions rg{};
  std::vector<LaneState> lanes;
  std::vector<NeedleHipRun> runs;
  // resident videos: K of them in front of the arriving ones; rows k * regions + r
  size_t residents = 0;
  std::vector<NeedleHipSeq> res_rows;               // (the offsets are the caller's arena's: only the lengths are used)
  std::vector<std::vector<NeedleHipRun>> held;      // per lane: runs into a resident's last row, held back until it finishes
  DeviceBuffer<CrossLive> d_live;
  DeviceBuffer<CrossResident> d_resident;
  DeviceBuffer<uint32_t> hist, d_round;
  DeviceBuffer<uint8_t> state;
  PinnedStage round_stage;
  RunSlab<NeedleHipRun> slab;
  Origin origin;
  int device = 0;
  Status poison = Status::Ok();
  uint64_t feeds = 0, launches = 0, cells = 0;

  ~Impl() {
    std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
    round_stage.release();
    slab.head_stage.release();
  }

  // Is this run one into a resident's last row (crossmatch_walk_kernel hands those out early)?  A resident source is a video
  // below K of the pair that NeedleHipRun.problem names (pair_ids.h, through the plan's tables).
  bool into_a_residents_last_row(const NeedleHipRun &run, size_t *lane) const {
    uint32_t a = 0, b = 0, r = 0;
    if (!residents || !plan.problem_at(run.problem, &a, &b, &r) || a >= residents) return false;
    *lane = (size_t)((b - residents) * regions + r);
    return (uint64_t)run.src_end + 1 == res_rows[a * regions + r].len;
  }
  size_t capacity_of(size_t lane) const { return max_items[lane % regions]; }

  // cells of all live problems when the lanes hold `fed` (+ `pieces`)
  uint64_t cells_of(const std::vector<Piece> *pieces) const {
    return plan.cells([&](size_t i) { return std::max<uint64_t>(lanes[i].fed + (pieces ? (*pieces)[i].width : 0u), 1) - 1; });
  }

  // One round over `pieces` (one per lane).
  Status round(const std::vector<Piece> &pieces) {
    std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
    Status s = ensure_device();
    if (!s.ok()) return s;
    hipStream_t stream = library_stream();
    std::vector<CrossLane> lt(n);
    uint64_t words = n * (sizeof(CrossLane) / 4), longest = std::max<uint64_t>(plan.longest_resident, 1);
    for (size_t i = 0; i < n; i++) {
      const LaneState &l = lanes[i];
      lt[i] = CrossLane{(uint32_t)l.fed, pieces[i].width, (uint32_t)words,
                        l.parity | (l.finished ? kFinished : 0u) | (pieces[i].finishing ? kFinishing : 0u)};
      words += pieces[i].width;
      longest = std::max(longest, l.fed + pieces[i].width);
    }
    const uint64_t round_cells = cells_of(&pieces) - cells_of(nullptr);
    if (!(s = upload_round(lt, pieces, words, &d_round, &round_stage, stream)).ok()) return s;

    const CrossLane *d_lanes = reinterpret_cast<const CrossLane *>(d_round.ptr);
    const dim3 block(kThreads);
    const uint32_t side_blocks = (uint32_t)((longest + kCarriedRows - 1) / kCarriedRows);  // of the longest lane or resident row of any region: the others' leave at once
    const uint32_t problems = (uint32_t)plan.problems();  // (a labelling without live pairs still launches one row of workgroups)
    const dim3 walk_grid(2u * (side_blocks + kTopBlocks), std::max(problems, 1u));
    std::vector<NeedleHipRun> got;
    for (;;) {
      uint32_t *d_count = nullptr;
      NeedleHipRun *d_runs = nullptr;
      if (!(s = slab.begin(&d_count, &d_runs)).ok()) return s;
      {
        KernelTimer timer("crossmatch_land");
        hipLaunchKernelGGL(crossmatch_land_kernel, dim3(kMaxStrip / kThreads, (uint32_t)n), block, 0, stream, d_round.ptr, hist.ptr,
                           rg, d_count);
        NEEDLE_HIP_TRY(hipGetLastError());
      }
      {
        KernelTimer timer("crossmatch_walk");
        if (plan.labelled && plan.narrow)
          hipLaunchKernelGGL((crossmatch_walk_kernel<uint16_t, ListedLivePairs, const CrossLive *, uint32_t>), walk_grid, block, 0, stream, hist.ptr,
                             reinterpret_cast<uint16_t *>(state.ptr), d_lanes, (const CrossResident *)d_resident.ptr, (uint32_t)videos, rg,
                             side_blocks, threshold, d_runs, slab.capacity, d_count, (const CrossLive *)d_live.ptr, problems);
        else if (plan.labelled)
          hipLaunchKernelGGL((crossmatch_walk_kernel<uint32_t, ListedLivePairs, const CrossLive *, uint32_t>), walk_grid, block, 0, stream, hist.ptr,
                             reinterpret_cast<uint32_t *>(state.ptr), d_lanes, (const CrossResident *)d_resident.ptr, (uint32_t)videos, rg,
                             side_blocks, threshold, d_runs, slab.capacity, d_count, (const CrossLive *)d_live.ptr, problems);
        else if (plan.narrow)
          hipLaunchKernelGGL((crossmatch_walk_kernel<uint16_t, ClosedFormPairs>), walk_grid, block, 0, stream, hist.ptr,
                             reinterpret_cast<uint16_t *>(state.ptr), d_lanes, d_resident.ptr, (uint32_t)videos, rg, side_blocks, threshold, d_runs,
                             slab.capacity, d_count);
        else
          hipLaunchKernelGGL((crossmatch_walk_kernel<uint32_t, ClosedFormPairs>), walk_grid, block, 0, stream, hist.ptr,
                             reinterpret_cast<uint32_t *>(state.ptr), d_lanes, d_resident.ptr, (uint32_t)videos, rg, side_blocks, threshold, d_runs,
                             slab.capacity, d_count);
        NEEDLE_HIP_TRY(hipGetLastError());
      }
      {
        KernelTimer timer("crossmatch_simhash");
        hipLaunchKernelGGL(crossmatch_simhash_kernel, dim3((uint32_t)device_cu_count() * 2u), block, 0, stream, hist.ptr, d_resident.ptr,
                           rg, d_runs, slab.capacity, d_count);
        NEEDLE_HIP_TRY(hipGetLastError());
      }
      launches += 3;
      cells += round_cells;
      bool again = false;  // a larger slab, and the round again (it wrote nothing that it reads)
      if (!(s = slab.collect(stream, &got, &again)).ok()) return s;
      round_stage.pending = false;
      if (!again) break;
    }
    // What is open on a frontier is reported when the pair becomes complete: a run into a resident's last row waits for its
    // lane's finish round (the kernel kept no state for it).
    for (const NeedleHipRun &run : got) {
      size_t lane = 0;
      if (into_a_residents_last_row(run, &lane) && !pieces[lane].finishing) held[lane].push_back(run);
      else runs.push_back(run);
    }
    for (size_t i = 0; i < n; i++) {
      LaneState &l = lanes[i];
      l.fed += pieces[i].width;
      if (pieces[i].width) l.parity ^= kParity;
      if (pieces[i].finishing) {
        l.finished = true;
        runs.insert(runs.end(), held[i].begin(), held[i].end());
        held[i] = std::vector<NeedleHipRun>();
      }
    }
    return Status::Ok();
  }

  Status guarded_round(const std::vector<Piece> &pieces) { return poison_on_failure(round(pieces), &poison); }
};

CrossMatcher::CrossMatcher() : impl_(new Impl()) {}
CrossMatcher::~CrossMatcher() = default;
size_t CrossMatcher::lanes() const { return impl_->n; }

size_t CrossMatcher::videos() const { return impl_->videos; }
size_t CrossMatcher::regions() const { return impl_->regions; }

size_t CrossMatcher::residents() const { return impl_->residents; }

size_t CrossMatcher::StateBytes(const Spec &spec) {
  const CrossPairsPlan plan = plan_cross_pairs(spec);
  return plan.error ? 0 : plan.state_bytes();
}

const char *CrossMatcher::ShapeError(const Spec &spec) { return plan_cross_pairs(spec).error; }

// The one way in: the plan of cross_pairs.h, executed.  The resident hashes reach the histories packed on the host and uploaded,
// or gathered from a device arena; only the residents that are in a live pair have hashes here (the device table says len 0 for
// the others: nothing of them is copied or gathered), and a labelled object's live-pair table goes up next to the resident table.
Status CrossMatcher::Create(Spec spec, const uint32_t *hashes, size_t num_hashes, bool on_device, std::unique_ptr<CrossMatcher> *out) {
  const size_t K = spec.residents, regions = spec.regions;
  if (!out || !spec.max_items || !spec.min_len || (K && (!spec.resident || (spec.groups && !spec.resident_groups))) || (num_hashes && !hashes))
    return Status::Make(NeedleError_NullArgument, "crossmatcher: null argument");
  spec.arena_hashes = num_hashes;
  CrossPairsPlan plan = plan_cross_pairs(spec);
  if (plan.error) return Status::Make(NeedleError_InvalidArgument, plan.error);
  std::unique_ptr<CrossMatcher> cm(new CrossMatcher());
  Impl &m = *cm->impl_;
  m.videos = spec.arriving;
  m.regions = regions;
  m.residents = K;
  m.n = spec.arriving * regions;
  m.threshold = spec.threshold;
  m.lanes = std::vector<LaneState>(m.n);
  m.held.resize(m.n);
  m.res_rows.assign(spec.resident, spec.resident + K * regions);
  std::vector<CrossResident> table(K * regions);
  for (size_t i = 0; i < table.size(); i++)
    table[i] = CrossResident{plan.resident_prefix[i], plan.resident_live[i / regions] ? spec.resident[i].len : 0u, spec.resident[i].offset};
  for (size_t r = 0; r < regions; r++) {
    m.max_items[r] = spec.max_items[r];
    m.min_len[r] = spec.min_len[r];
  }
  m.rg.regions = (uint32_t)regions;
  m.rg.residents = (uint32_t)K;
  m.rg.max_items0 = (uint32_t)m.max_items[0];
  m.rg.max_items1 = (uint32_t)m.max_items[regions - 1];
  m.rg.min_len0 = m.min_len[0];
  m.rg.min_len1 = m.min_len[regions - 1];
  m.rg.hist0 = plan.hist[0];
  m.rg.hist1 = plan.hist[regions - 1];
  m.rg.state0 = plan.state[0];
  m.rg.state1 = plan.state[regions - 1];
  m.rg.res_hist0 = plan.res_hist[0];
  m.rg.res_hist1 = plan.res_hist[regions - 1];
  m.rg.res_state0 = plan.res_state[0];  // (the closed form's, as res_total: a listed problem's state is in its table entry)
  m.rg.res_state1 = plan.res_state[regions - 1];
  m.rg.res_total0 = plan.resident_hashes[0];
  m.rg.res_total1 = plan.resident_hashes[regions - 1];
  if (!plan.labelled) std::vector<CrossLive>().swap(plan.live);  // the closed form finds them by arithmetic
  m.plan = std::move(plan);
  const CrossPairsPlan &pl = m.plan;
  m.slab.capacity_from_env("NEEDLE_HIP_CROSSMATCHER_RUN_SLAB");

  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = ensure_device();
  if (!s.ok()) return s;
  hipStream_t stream = library_stream();
  const size_t state_bytes = (size_t)pl.state_entries * pl.entry_bytes(), first_resident_word = (size_t)pl.res_hist[0];
  if (!(s = m.hist.reserve(std::max<size_t>(pl.hist_words, 1))).ok() || !(s = m.state.reserve(std::max<size_t>(state_bytes, 1))).ok() ||
      !(s = m.d_live.reserve(pl.labelled ? std::max<size_t>(pl.live.size(), 1) : 0)).ok())
    return s;
  if (state_bytes) NEEDLE_HIP_TRY(hipMemsetAsync(m.state.ptr, 0, state_bytes, stream));
  (void)hipGetDevice(&m.device);
  if (!pl.live.empty())
    NEEDLE_HIP_TRY(hipMemcpyAsync(m.d_live.ptr, pl.live.data(), pl.live.size() * sizeof(CrossLive), hipMemcpyHostToDevice, stream));
  if (K) {  // the table, and the rows in table order behind the histories: this once
    if (!(s = m.d_resident.reserve(table.size())).ok()) return s;
    NEEDLE_HIP_TRY(hipMemcpyAsync(m.d_resident.ptr, table.data(), table.size() * sizeof(CrossResident), hipMemcpyHostToDevice, stream));
    if (on_device) {
      KernelTimer timer("crossmatch_gather_resident", stream);
      if (pl.hist_words > first_resident_word)
        hipLaunchKernelGGL(crossmatch_gather_resident_kernel, dim3((uint32_t)std::min<size_t>(table.size(), 4096)), dim3(kThreads), 0, stream,
                           hashes, (const CrossResident *)m.d_resident.ptr, (uint32_t)table.size(), m.rg, m.hist.ptr);
      NEEDLE_HIP_TRY(hipGetLastError());
    } else {
      std::vector<uint32_t> packed(pl.hist_words - first_resident_word);
      for (size_t i = 0; i < table.size(); i++)
        if (table[i].len)
          std::memcpy(packed.data() + (pl.res_hist[i % regions] - first_resident_word) + table[i].prefix, hashes + spec.resident[i].offset,
                      (size_t)table[i].len * sizeof(uint32_t));
      if (!packed.empty())
        NEEDLE_HIP_TRY(hipMemcpyAsync(m.hist.ptr + first_resident_word, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
      NEEDLE_HIP_TRY(hipStreamSynchronize(stream));  // (before `packed` goes)
    }
  }
  NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  *out = std::move(cm);
  return Status::Ok();
}

bool CrossMatcher::grouped() const { return impl_->plan.labelled; }
const std::vector<uint32_t> &CrossMatcher::labels() const { return impl_->plan.labels; }

Status CrossMatcher::Feed(const uint32_t *const *items, const size_t *num_items) {
  Impl &m = *impl_;
  if (!items || !num_items) return Status::Make(NeedleError_NullArgument, "crossmatcher: null argument");
  if (!m.poison.ok()) return m.poison;
  bool any = false;
  for (size_t i = 0; i < m.n; i++) {
    if (!num_items[i]) continue;
    if (m.lanes[i].finished) return Status::Make(NeedleError_InvalidArgument, "crossmatcher: the lane is finished");
    if (!items[i]) return Status::Make(NeedleError_NullArgument, "crossmatcher: null chunk");
    if (num_items[i] > m.capacity_of(i) - m.lanes[i].fed) return Status::Make(NeedleError_InvalidArgument, "crossmatcher: more than max_items in a lane");
    any = true;
  }
  if (!any) return Status::Ok();
  m.feeds++;
  std::vector<size_t> done(m.n, 0);
  for (;;) {  // a feed of more than a strip for one lane is cut into rounds
    std::vector<Piece> pieces(m.n);
    bool more = false;
    for (size_t i = 0; i < m.n; i++) {
      const size_t take = std::min<size_t>(num_items[i] - done[i], kMaxStrip);
      if (take) pieces[i] = Piece{items[i] + done[i], (uint32_t)take, false};
      done[i] += take;
      more = more || done[i] < num_items[i];
    }
    Status s = m.guarded_round(pieces);
    if (!s.ok() || !more) return s;
  }
}

Status CrossMatcher::FeedFromFeeder(Feeder *feeder) {
  Impl &m = *impl_;
  FeederTake take;
  Status s = take_from_feeder(
      feeder, m.n, m.poison, [&](size_t i, uint64_t *fed, bool *finished) { *fed = m.lanes[i].fed, *finished = m.lanes[i].finished; },
      "crossmatcher: ", "", &take);
  if (!s.ok()) return s;
  s = Feed(take.ptrs.data(), take.counts.data());
  if (!s.ok() || take.finish.empty()) return s;
  return Finish(take.finish.data(), take.finish.size());
}

Status CrossMatcher::Finish(const size_t *lanes, size_t k) {
  Impl &m = *impl_;
  if (!m.poison.ok()) return m.poison;
  std::vector<Piece> pieces(m.n);
  bool any = false;
  for (size_t j = 0; j < (lanes ? k : m.n); j++) {
    const size_t i = lanes ? lanes[j] : j;
    if (i >= m.n) return Status::Make(NeedleError_InvalidArgument, "crossmatcher: lane out of range");
    if (m.lanes[i].finished) continue;
    pieces[i].finishing = any = true;
  }
  if (!any) return Status::Ok();
  return m.guarded_round(pieces);
}

Status CrossMatcher::Ready(size_t *num_runs, bool *complete) {
  Impl &m = *impl_;
  if (!m.poison.ok()) return m.poison;
  if (num_runs) *num_runs = m.runs.size();
  if (complete) *complete = std::all_of(m.lanes.begin(), m.lanes.end(), [](const LaneState &l) { return l.finished; });
  return Status::Ok();
}

Status CrossMatcher::Lane(size_t lane, uint64_t *items_fed, bool *finished) {
  Impl &m = *impl_;
  if (lane >= m.n) return Status::Make(NeedleError_InvalidArgument, "crossmatcher: lane out of range");
  if (!m.poison.ok()) return m.poison;
  if (items_fed) *items_fed = m.lanes[lane].fed;
  if (finished) *finished = m.lanes[lane].finished;
  return Status::Ok();
}

Status CrossMatcher::Runs(size_t first, size_t count, NeedleHipRun *runs) {
  size_t have = 0;
  Status s = Ready(&have, nullptr);
  if (!s.ok()) return s;
  if (first > have || count > have - first) return Status::Make(NeedleError_InvalidArgument, "crossmatcher: runs out of range");
  if (count && !runs) return Status::Make(NeedleError_NullArgument, "crossmatcher: null argument");
  if (count) std::memcpy(runs, impl_->runs.data() + first, count * sizeof(NeedleHipRun));
  return Status::Ok();
}

void CrossMatcher::set_origin(const Origin &origin) { impl_->origin = origin; }
CrossMatcher::Origin CrossMatcher::origin() const { return impl_->origin; }
int CrossMatcher::device() const { return impl_->device; }
uint32_t CrossMatcher::min_len(size_t region) const { return impl_->min_len[region < kCrossMaxRegions ? region : 0]; }
Status CrossMatcher::poisoned() const { return impl_->poison; }
const std::vector<NeedleHipRun> &CrossMatcher::run_list() const { return impl_->runs; }
const uint32_t *CrossMatcher::history(size_t lane) const {
  const Impl &m = *impl_;
  const size_t r = lane % m.regions;
  return m.hist.ptr + (r ? m.rg.hist1 : m.rg.hist0) + (lane / m.regions) * m.max_items[r];
}

void CrossMatcher::Stats(uint64_t stats[4]) const {
  const Impl &m = *impl_;
  stats[0] = m.feeds;
  stats[1] = m.launches;
  stats[2] = m.cells;
  // frontiers and hashes by the plan's rule, the two tables as uploaded, the run slab
  stats[3] = m.plan.state_bytes() + m.plan.live.size() * sizeof(CrossLive) + m.res_rows.size() * sizeof(CrossResident) + m.slab.bytes();
}

}  // namespace needle
