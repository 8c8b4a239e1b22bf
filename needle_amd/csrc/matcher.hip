// Streaming comparator (include/needle_hip.h needle_hip_matcher_*): the search half of the streaming path.  S source
// sequences are resident in HBM; N lanes are destination sequences whose hashes arrive in chunks; a feed evaluates the
// cells of its new columns only and reports the runs those columns close, exactly the runs (and simhashes) that
// needle_hip_hamming_runs_host finds over the concatenation of a lane's chunks.
//
// This is stream_walk.h's walk in its column direction with X = a source, complete, and Y = the lane.  State of a (lane,
// source): the frontier along the last column fed, one run length per source row (u16 where every source is shorter than
// 65 536 hashes, else u32), in two sets of buffers: a round reads one and writes the other.  Per lane, its hashes so far.
//
// One round (a feed, or a strip of one that is wider than kMaxStrip columns; also `finish` and `open`, with no columns) is
// three launches whatever N and S -- matcher_land_kernel, matcher_strip_kernel, matcher_simhash_kernel: every kernel finds
// its lane in the round's lane table (blockIdx.y) and its source in the resident source table (through the resident list of
// every workgroup's source, blockIdx.x); only the lanes with data are in the grid.
//
// Regions (CreateRegions; needle_hip_matcher_new_regions): source s is in region s % regions, lane l in region l % regions,
// and a lane meets the sources of its own region only.  The source table and the workgroup list are ordered by region; a lane
// table entry names its region's first workgroup and workgroup count, and its state holds its own region's frontiers alone.
// The grid's x is the larger workgroup count of the regions in the round: a workgroup beyond its lane's region leaves after
// the lane table read, so a round stays three launches.  One region is the kernel without any of this (kRegions = false).
#include "matcher.h"

#include <algorithm>
#include <cstring>

#include "stream_round.h"
#include "stream_walk.h"

namespace needle {

namespace {

constexpr uint32_t kEmitOpen = 1u;  // no state is written: what is open on the frontier is reported (finish, open)
constexpr uint32_t kNoHash = 2u;    // the runs keep zero simhashes (open)

// A source's workgroups: ceil((n - 1) / kCarriedRows) of carried diagonals, then kTopBlocks of entering ones.  The count is
// that of the widest strip, so the tables (sources, and the source of every workgroup) are built once.
struct MatchSource {
  uint32_t src_off, n;  // arena offset and length (>= 2)
  uint32_t min_len, index;
  uint32_t row_off;     // of the source's rows inside a lane's state (its region's part of it)
  uint32_t block_base, carried_blocks;
  uint32_t from_off;    // where the row lay in the device arena it was gathered from (matcher_gather_kernel; no round reads it)
};

struct MatchLane {
  uint32_t *hist;    // the lane's hashes so far
  const void *from;  // state set the round reads ...
  void *to;          // ... and the one it writes
  uint32_t fed, width;      // J and the strip's columns [J, J + width)
  uint32_t stage_off;       // of the new hashes inside the round's buffer, in words
  uint32_t flags;
  uint32_t block_first, blocks;  // the workgroups of the lane's region in the workgroup list (read with regions only)
};
static_assert(sizeof(MatchLane) == 48, "lane table entries are 12 words");

struct MatchRun {  // NeedleHipRun, of the source's table entry, + the lane's slot in the round's table: the host resolves both
  uint32_t problem, src_end, dst_end, len, src_match_hash, dst_match_hash, lane, pad;
};

__global__ __launch_bounds__(kThreads) void matcher_land_kernel(const uint32_t *__restrict__ round_buf, uint32_t *__restrict__ count) {
  land_chunks<MatchLane>(round_buf, count, [](const MatchLane &ln) { return ln.hist; });
}

// Sources from an arena in device memory (the index store's) into the matcher's own, packed in table order: a workgroup per
// source, consecutive lanes move consecutive words.  Creation checked every source against the arena.
__global__ __launch_bounds__(kThreads) void matcher_gather_kernel(const uint32_t *__restrict__ from, const MatchSource *__restrict__ sources,
                                                                  uint32_t num_sources, uint32_t *__restrict__ arena) {
  for (uint32_t s = blockIdx.x; s < num_sources; s += gridDim.x) {
    const MatchSource sc = sources[s];
    for (uint32_t k = threadIdx.x; k < sc.n; k += kThreads) arena[sc.src_off + k] = from[sc.from_off + k];
  }
}

template <typename T, bool kRegions>
__global__ __launch_bounds__(kThreads) void matcher_strip_kernel(const uint32_t *__restrict__ arena,
                                                                 const MatchSource *__restrict__ sources,
                                                                 const uint32_t *__restrict__ block_source,
                                                                 const MatchLane *__restrict__ lanes, uint32_t threshold,
                                                                 MatchRun *__restrict__ runs, uint32_t capacity,
                                                                 uint32_t *__restrict__ count) {
  __shared__ uint32_t strip[kMaxStrip];                // dst[J .. J + W)
  __shared__ uint32_t rows[kCarriedRows + kMaxStrip];  // the source rows this workgroup's diagonals meet
  const MatchLane ln = lanes[blockIdx.y];
  uint32_t blk = blockIdx.x;
  if (kRegions) {  // the workgroups of the lane's region; the grid is as wide as the larger region (the whole workgroup leaves)
    if (blk >= ln.blocks) return;
    blk += ln.block_first;
  }
  const uint32_t lo = block_source[blk];
  const MatchSource sc = sources[lo];
  // a lane that holds fewer than two items has no cell yet, whatever a reset left in its sets
  const WalkSide<T> sd{arena + sc.src_off, ln.hist, sc.n, max(ln.fed, 1u), max(ln.fed + ln.width, 1u), sc.n - 1u,
                       ln.fed >= 2u ? static_cast<const T *>(ln.from) + sc.row_off : nullptr, static_cast<T *>(ln.to) + sc.row_off, nullptr, true};
  stream_walk<T, true>(strip, rows, sd, blk - sc.block_base, sc.carried_blocks, (ln.flags & kEmitOpen) != 0u, threshold, sc.min_len, runs,
                       capacity, count, [&](const uint32_t src_end, const uint32_t dst_end, const uint32_t len) {
                         return MatchRun{lo, src_end, dst_end, len, 0u, 0u, blockIdx.y, 0u};
                       });
}

__global__ __launch_bounds__(kThreads) void matcher_simhash_kernel(const uint32_t *__restrict__ arena,
                                                                   const MatchSource *__restrict__ sources,
                                                                   const MatchLane *__restrict__ lanes,
                                                                   MatchRun *__restrict__ runs, uint32_t capacity,
                                                                   const uint32_t *__restrict__ count) {
  simhash_runs(
      runs, capacity, count,
      [&](const MatchRun &r) -> const uint32_t * { return lanes[r.lane].flags & kNoHash ? nullptr : arena + sources[r.problem].src_off; },
      [&](const MatchRun &r) -> const uint32_t * { return lanes[r.lane].flags & kNoHash ? nullptr : lanes[r.lane].hist; });
}

struct LaneState {
  uint64_t fed = 0;
  bool finished = false;
  int cur = 0;  // the set that holds the lane's state
  uint32_t *hist = nullptr;
  uint64_t hist_cap = 0;
  std::vector<NeedleHipRun> runs;
};

struct Piece {
  size_t lane;
  const uint32_t *items;
  uint32_t width, flags;
};

}  // namespace

struct Matcher::Impl {
  size_t n = 0;
  size_t regions = 1;
  uint32_t threshold = 0;
  bool narrow = true;       // u16 run lengths
  // Per region: the rows of a lane's state, the sum of n_s - 1, and its workgroups in the list.  A video's lanes lie side by
  // side in a set: lane l at (l / regions) * total_rows, region 1 behind region 0's rows.
  uint64_t region_rows[2] = {0, 0}, region_cells[2] = {0, 0};
  uint32_t region_first_block[2] = {0, 0}, region_blocks[2] = {0, 0};
  uint64_t total_rows = 0;  // of one video's lanes
  uint32_t total_blocks = 0;
  std::vector<MatchSource> table;  // the sources that have cells, region after region
  Matcher::Origin origin;
  int device = 0;
  std::vector<LaneState> lanes;
  DeviceBuffer<uint32_t> arena;
  DeviceBuffer<MatchSource> d_table;
  std::vector<uint32_t> block_source;  // the table entry of every workgroup of the scan's grid
  DeviceBuffer<uint32_t> d_block_source;
  DeviceBuffer<uint8_t> state[2];
  DeviceBuffer<uint32_t> d_round;
  PinnedStage round_stage;
  RunSlab<MatchRun> slab;
  Status poison = Status::Ok();
  uint64_t feeds = 0, launches = 0, cells = 0, arena_bytes = 0;

  ~Impl() {
    std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
    for (LaneState &l : lanes)
      if (l.hist) (void)hipFree(l.hist);
    round_stage.release();
    slab.head_stage.release();
  }

  size_t state_elem() const { return narrow ? sizeof(uint16_t) : sizeof(uint32_t); }
  size_t region_of(size_t lane) const { return lane % regions; }
  bool has_cells(size_t lane) const { return region_blocks[region_of(lane)] != 0; }  // else the lane only counts
  uint64_t state_off(size_t lane) const {  // of the lane's frontiers in a set, in bytes
    return ((uint64_t)(lane / regions) * total_rows + (region_of(lane) ? region_rows[0] : 0)) * state_elem();
  }
  uint64_t state_rows() const {  // of all lanes, one set
    return (uint64_t)(n / regions) * total_rows;
  }

  Status grow_history(LaneState &l, uint64_t need, hipStream_t stream) {
    if (need <= l.hist_cap) return Status::Ok();
    const uint64_t cap = std::max<uint64_t>({need, l.hist_cap * 2, 4096});
    uint32_t *p = nullptr;
    NEEDLE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), cap * sizeof(uint32_t)));
    if (l.hist) {
      hipError_t e = l.fed ? hipMemcpyAsync(p, l.hist, l.fed * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream) : hipSuccess;
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      if (e != hipSuccess) {
        (void)hipFree(p);
        NEEDLE_HIP_TRY(e);
      }
      (void)hipFree(l.hist);
    }
    l.hist = p;
    l.hist_cap = cap;
    return Status::Ok();
  }

  // One round over `pieces` (distinct lanes).  Runs go to their lanes' lists, or to *open_out (then nothing changes).
  Status round(const std::vector<Piece> &pieces, std::vector<NeedleHipRun> *open_out) {
    std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
    Status s = ensure_device();
    if (!s.ok()) return s;
    hipStream_t stream = library_stream();
    const size_t k = pieces.size();
    uint32_t widest = 0;
    uint64_t words = k * (sizeof(MatchLane) / 4);
    for (const Piece &p : pieces) {
      if (!(s = grow_history(lanes[p.lane], lanes[p.lane].fed + p.width, stream)).ok()) return s;
      widest = std::max(widest, p.width);
    }
    std::vector<MatchLane> lt(k);
    uint64_t round_cells = 0;
    uint32_t grid_blocks = 0;  // the most workgroups a lane of the round has
    for (size_t a = 0; a < k; a++) {
      const Piece &p = pieces[a];
      const LaneState &l = lanes[p.lane];
      const size_t r = region_of(p.lane);
      MatchLane &e = lt[a];
      e.hist = l.hist;
      e.from = state[l.cur].ptr + state_off(p.lane);
      e.to = state[l.cur ^ 1].ptr + state_off(p.lane);
      e.fed = (uint32_t)l.fed;
      e.width = p.width;
      e.stage_off = (uint32_t)words;
      e.flags = p.flags;
      e.block_first = region_first_block[r];
      e.blocks = region_blocks[r];
      grid_blocks = std::max(grid_blocks, region_blocks[r]);
      words += p.width;
      round_cells += region_cells[r] * (uint64_t)(p.width - (l.fed == 0 && p.width ? 1u : 0u));
    }
    if (!(s = upload_round(lt, pieces, words, &d_round, &round_stage, stream)).ok()) return s;

    const MatchLane *d_lanes = reinterpret_cast<const MatchLane *>(d_round.ptr);
    const dim3 block(kThreads);
    std::vector<MatchRun> got;
    for (;;) {
      uint32_t *d_count = nullptr;
      MatchRun *d_runs = nullptr;
      if (!(s = slab.begin(&d_count, &d_runs)).ok()) return s;
      {
        KernelTimer timer("matcher_land");
        hipLaunchKernelGGL(matcher_land_kernel, dim3((std::max(widest, 1u) + kThreads - 1) / kThreads, (uint32_t)k), block, 0, stream,
                           d_round.ptr, d_count);
        NEEDLE_HIP_TRY(hipGetLastError());
      }
      {
        KernelTimer timer("matcher_strip");
        const dim3 grid(grid_blocks, (uint32_t)k);  // (one region: total_blocks)
        auto launch = [&](auto kernel) {
          hipLaunchKernelGGL(kernel, grid, block, 0, stream, arena.ptr, d_table.ptr, d_block_source.ptr, d_lanes, threshold, d_runs,
                             slab.capacity, d_count);
        };
        if (regions == 1) narrow ? launch(matcher_strip_kernel<uint16_t, false>) : launch(matcher_strip_kernel<uint32_t, false>);
        else narrow ? launch(matcher_strip_kernel<uint16_t, true>) : launch(matcher_strip_kernel<uint32_t, true>);
        NEEDLE_HIP_TRY(hipGetLastError());
      }
      {
        KernelTimer timer("matcher_simhash");
        hipLaunchKernelGGL(matcher_simhash_kernel, dim3((uint32_t)device_cu_count() * 2u), block, 0, stream, arena.ptr, d_table.ptr, d_lanes,
                           d_runs, slab.capacity, d_count);
        NEEDLE_HIP_TRY(hipGetLastError());
      }
      launches += 3;
      cells += round_cells;
      bool again = false;  // a larger slab, and the round again from the set it did not write
      if (!(s = slab.collect(stream, &got, &again)).ok()) return s;
      round_stage.pending = false;
      if (!again) break;
    }
    for (const MatchRun &r : got) {
      const NeedleHipRun out{table[r.problem].index, r.src_end, r.dst_end, r.len, r.src_match_hash, r.dst_match_hash};
      if (open_out) open_out->push_back(out);
      else lanes[pieces[r.lane].lane].runs.push_back(out);
    }
    if (open_out) return Status::Ok();
    for (const Piece &p : pieces) {
      LaneState &l = lanes[p.lane];
      if (p.flags & kEmitOpen) {
        l.finished = true;
      } else {
        l.fed += p.width;
        l.cur ^= 1;
      }
    }
    return Status::Ok();
  }

  Status guarded_round(const std::vector<Piece> &pieces, std::vector<NeedleHipRun> *open_out) {
    return poison_on_failure(round(pieces, open_out), &poison);
  }
};

Matcher::Matcher() : impl_(new Impl()) {}
Matcher::~Matcher() = default;
size_t Matcher::lanes() const { return impl_->n; }

Status Matcher::Create(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len,
                       size_t num_sources, size_t lanes, uint32_t threshold, std::unique_ptr<Matcher> *out) {
  return CreateFrom(hashes, false, num_hashes, sources, min_len, false, num_sources, 1, lanes, threshold, out);
}

Status Matcher::CreateRegions(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len,
                              size_t num_sources, size_t regions, size_t lanes, uint32_t threshold, std::unique_ptr<Matcher> *out) {
  return CreateFrom(hashes, false, num_hashes, sources, min_len, true, num_sources, regions, lanes, threshold, out);
}

Status Matcher::CreateRegionsDevice(const uint32_t *d_hashes, size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len,
                                    size_t num_sources, size_t regions, size_t lanes, uint32_t threshold, std::unique_ptr<Matcher> *out) {
  return CreateFrom(d_hashes, true, num_hashes, sources, min_len, true, num_sources, regions, lanes, threshold, out);
}

Status Matcher::CheckShape(size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len, size_t num_sources, size_t regions,
                           size_t lanes) {
  if (!sources || !min_len) return Status::Make(NeedleError_NullArgument, "matcher: null argument");
  Impl scratch;
  return Plan(&scratch, false, num_hashes, sources, min_len, true, num_sources, regions, lanes);
}

// The argument checks and the tables, host arithmetic alone.  `packed`: the arena will hold the sources with cells only, in
// table order (gathered from a device arena); otherwise it is the caller's, offsets and all.
Status Matcher::Plan(Impl *impl, bool packed, size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len, bool min_len_zero_ok,
                     size_t num_sources, size_t regions, size_t lanes) {
  Impl &m = *impl;
  if (regions < 1 || regions > 2) return Status::Make(NeedleError_InvalidArgument, "matcher: regions must be 1 or 2");
  if (lanes == 0 || lanes > 65535) return Status::Make(NeedleError_InvalidArgument, "matcher: lanes must be 1 to 65535");
  if (num_sources == 0 || num_sources > 0xFFFFFFFFull || num_hashes > 0xFFFFFFFFull)
    return Status::Make(NeedleError_InvalidArgument, "matcher: 1 to 2^32 - 1 sources inside at most 2^32 - 1 hashes");
  if (num_sources % regions || lanes % regions)
    return Status::Make(NeedleError_InvalidArgument, "matcher: the sources and the lanes must be multiples of the regions");
  uint64_t blocks = 0, packed_hashes = 0;
  for (size_t r = 0; r < regions; r++) {  // the table and the workgroup list region after region (one region: the sources in order)
    m.region_first_block[r] = (uint32_t)blocks;
    for (size_t s = r; s < num_sources; s += regions) {
      if (min_len[s] == 0 && !min_len_zero_ok) return Status::Make(NeedleError_InvalidArgument, "matcher: min_len must be >= 1");
      if ((uint64_t)sources[s].offset + sources[s].len > num_hashes) return Status::Make(NeedleError_InvalidArgument, "matcher: a source lies outside the hashes");
      const uint32_t len = sources[s].len;
      if (len >= 65536) m.narrow = false;
      if (len >= 2 && min_len[s] != 0) {  // a shorter source, or one that can hold no run, has no cells
        MatchSource e{};
        e.src_off = packed ? (uint32_t)packed_hashes : sources[s].offset;
        e.from_off = sources[s].offset;
        e.n = len;
        e.min_len = min_len[s];
        e.index = (uint32_t)s;
        e.row_off = (uint32_t)m.region_rows[r];
        e.block_base = (uint32_t)blocks;
        e.carried_blocks = (len - 1 + kCarriedRows - 1) / kCarriedRows;
        blocks += e.carried_blocks + kTopBlocks;
        packed_hashes += len;
        m.region_rows[r] += len;
        m.region_cells[r] += len - 1;
        m.total_rows += len;
        m.block_source.insert(m.block_source.end(), e.carried_blocks + kTopBlocks, (uint32_t)m.table.size());
        m.table.push_back(e);
      }
      if (blocks > 0x7FFFFFFFull || m.total_rows > 0xFFFFFFFFull) return Status::Make(NeedleError_InvalidArgument, "matcher: the sources are too long together");
    }
    m.region_blocks[r] = (uint32_t)blocks - m.region_first_block[r];
  }
  m.n = lanes;
  m.regions = regions;
  m.total_blocks = (uint32_t)blocks;
  m.arena_bytes = m.table.empty() ? 0 : (packed ? packed_hashes : (uint64_t)num_hashes) * sizeof(uint32_t);  // (no cells: nothing goes up)
  return Status::Ok();
}

// Every way in shares everything but how the sources reach the arena: the caller's host arena uploaded whole, or the sources
// with cells gathered from a device arena (the index store's), no hashes uploaded.
Status Matcher::CreateFrom(const uint32_t *hashes, bool on_device, size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len,
                           bool min_len_zero_ok, size_t num_sources, size_t regions, size_t lanes, uint32_t threshold,
                           std::unique_ptr<Matcher> *out) {
  if (!sources || !min_len || !out || (num_hashes && !hashes)) return Status::Make(NeedleError_NullArgument, "matcher: null argument");
  std::unique_ptr<Matcher> mt(new Matcher());
  Impl &m = *mt->impl_;
  Status s = Plan(&m, on_device, num_hashes, sources, min_len, min_len_zero_ok, num_sources, regions, lanes);
  if (!s.ok()) return s;
  m.threshold = threshold;
  m.lanes = std::vector<LaneState>(lanes);
  m.slab.capacity_from_env("NEEDLE_HIP_MATCHER_RUN_SLAB");

  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  if (!(s = ensure_device()).ok()) return s;
  (void)hipGetDevice(&m.device);
  if (!m.table.empty()) {
    hipStream_t stream = library_stream();
    const uint64_t state_bytes = m.state_rows() * m.state_elem();
    if (!(s = m.arena.reserve(std::max<size_t>(m.arena_bytes / sizeof(uint32_t), 1))).ok() || !(s = m.d_table.reserve(m.table.size())).ok() ||
        !(s = m.d_block_source.reserve(m.block_source.size())).ok() ||
        !(s = m.state[0].reserve(state_bytes)).ok() || !(s = m.state[1].reserve(state_bytes)).ok())
      return s;
    NEEDLE_HIP_TRY(hipMemcpyAsync(m.d_table.ptr, m.table.data(), m.table.size() * sizeof(MatchSource), hipMemcpyHostToDevice, stream));
    if (on_device) {
      KernelTimer timer("matcher_gather", stream);
      hipLaunchKernelGGL(matcher_gather_kernel, dim3((uint32_t)std::min<size_t>(m.table.size(), 4096)), dim3(kThreads), 0, stream, hashes,
                         (const MatchSource *)m.d_table.ptr, (uint32_t)m.table.size(), m.arena.ptr);
      NEEDLE_HIP_TRY(hipGetLastError());
    } else {
      NEEDLE_HIP_TRY(hipMemcpyAsync(m.arena.ptr, hashes, num_hashes * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    }
    NEEDLE_HIP_TRY(hipMemcpyAsync(m.d_block_source.ptr, m.block_source.data(), m.block_source.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    NEEDLE_HIP_TRY(hipMemsetAsync(m.state[0].ptr, 0, state_bytes, stream));
    NEEDLE_HIP_TRY(hipMemsetAsync(m.state[1].ptr, 0, state_bytes, stream));
    NEEDLE_HIP_TRY(hipStreamSynchronize(stream));  // the caller's arrays are free on return
  }
  *out = std::move(mt);
  return Status::Ok();
}

Status Matcher::Feed(const uint32_t *const *items, const size_t *num_items) {
  Impl &m = *impl_;
  if (!items || !num_items) return Status::Make(NeedleError_NullArgument, "matcher: null argument");
  if (!m.poison.ok()) return m.poison;
  bool any = false;
  for (size_t i = 0; i < m.n; i++) {
    if (!num_items[i]) continue;
    if (m.lanes[i].finished) return Status::Make(NeedleError_InvalidArgument, "matcher: the lane is finished (reset it first)");
    if (!items[i]) return Status::Make(NeedleError_NullArgument, "matcher: null chunk");
    if (m.lanes[i].fed + num_items[i] > 0x7FFFFFF0ull) return Status::Make(NeedleError_InvalidArgument, "matcher: more than 2^31 items in a lane");
    any = true;
  }
  if (!any) return Status::Ok();
  m.feeds++;
  std::vector<size_t> done(m.n, 0);
  for (;;) {  // a feed wider than a strip is cut into rounds
    std::vector<Piece> pieces;
    bool more = false;
    for (size_t i = 0; i < m.n; i++) {
      const size_t take = std::min<size_t>(num_items[i] - done[i], kMaxStrip);
      if (take) {
        LaneState &l = m.lanes[i];
        if (!m.has_cells(i)) {  // no source of its region has a cell: the lane only counts
          l.fed += take;
        } else {
          pieces.push_back(Piece{i, items[i] + done[i], (uint32_t)take, 0u});
        }
        done[i] += take;
      }
      more = more || done[i] < num_items[i];
    }
    if (!pieces.empty()) {
      Status s = m.guarded_round(pieces, nullptr);
      if (!s.ok()) return s;
    }
    if (!more) return Status::Ok();
  }
}

Status Matcher::FeedFromFeeder(Feeder *feeder) {
  Impl &m = *impl_;
  FeederTake take;
  Status s = take_from_feeder(
      feeder, m.n, m.poison, [&](size_t i, uint64_t *fed, bool *finished) { *fed = m.lanes[i].fed, *finished = m.lanes[i].finished; }, "matcher: ",
      " (reset it first)", &take);
  if (!s.ok()) return s;
  s = Feed(take.ptrs.data(), take.counts.data());
  if (!s.ok() || take.finish.empty()) return s;
  return Finish(take.finish.data(), take.finish.size());
}

Status Matcher::Finish(const size_t *lanes, size_t k) {
  Impl &m = *impl_;
  if (!m.poison.ok()) return m.poison;
  std::vector<Piece> pieces;
  std::vector<bool> seen(m.n, false);
  for (size_t j = 0; j < (lanes ? k : m.n); j++) {
    const size_t i = lanes ? lanes[j] : j;
    if (i >= m.n) return Status::Make(NeedleError_InvalidArgument, "matcher: lane out of range");
    if (m.lanes[i].finished || seen[i]) continue;
    seen[i] = true;
    pieces.push_back(Piece{i, nullptr, 0u, kEmitOpen});
  }
  std::vector<Piece> walked;
  for (const Piece &p : pieces) {
    if (m.has_cells(p.lane)) walked.push_back(p);
    else m.lanes[p.lane].finished = true;  // (nothing can be open)
  }
  if (walked.empty()) return Status::Ok();
  return m.guarded_round(walked, nullptr);
}

Status Matcher::Reset(const size_t *lanes, size_t k) {
  Impl &m = *impl_;
  if (!m.poison.ok()) return m.poison;
  for (size_t j = 0; j < (lanes ? k : m.n); j++)
    if (lanes && lanes[j] >= m.n) return Status::Make(NeedleError_InvalidArgument, "matcher: lane out of range");
  for (size_t j = 0; j < (lanes ? k : m.n); j++) {
    LaneState &l = m.lanes[lanes ? lanes[j] : j];
    l.fed = 0;  // (a lane with no items never reads its carried lengths)
    l.finished = false;
    l.runs.clear();
  }
  return Status::Ok();
}

Status Matcher::Ready(size_t lane, size_t *num_runs, uint64_t *items_fed, bool *finished) {
  Impl &m = *impl_;
  if (lane >= m.n) return Status::Make(NeedleError_InvalidArgument, "matcher: lane out of range");
  if (!m.poison.ok()) return m.poison;
  if (num_runs) *num_runs = m.lanes[lane].runs.size();
  if (items_fed) *items_fed = m.lanes[lane].fed;
  if (finished) *finished = m.lanes[lane].finished;
  return Status::Ok();
}

Status Matcher::Runs(size_t lane, size_t first, size_t count, NeedleHipRun *runs) {
  size_t have = 0;
  Status s = Ready(lane, &have, nullptr, nullptr);
  if (!s.ok()) return s;
  if (first > have || count > have - first) return Status::Make(NeedleError_InvalidArgument, "matcher: runs out of range");
  if (count && !runs) return Status::Make(NeedleError_NullArgument, "matcher: null argument");
  if (count) std::memcpy(runs, impl_->lanes[lane].runs.data() + first, count * sizeof(NeedleHipRun));
  return Status::Ok();
}

Status Matcher::Open(size_t lane, std::vector<NeedleHipRun> *runs) {
  Impl &m = *impl_;
  if (lane >= m.n) return Status::Make(NeedleError_InvalidArgument, "matcher: lane out of range");
  if (!m.poison.ok()) return m.poison;
  runs->clear();
  if (m.lanes[lane].finished || m.lanes[lane].fed == 0 || !m.has_cells(lane)) return Status::Ok();  // nothing is open
  return m.guarded_round({Piece{lane, nullptr, 0u, kEmitOpen | kNoHash}}, runs);
}

void Matcher::Stats(uint64_t stats[4]) const {
  const Impl &m = *impl_;
  uint64_t history = 0;
  for (const LaneState &l : m.lanes) history += l.fed * sizeof(uint32_t);
  stats[0] = m.feeds;
  stats[1] = m.launches;
  stats[2] = m.cells;
  stats[3] = m.arena_bytes + 2 * m.state_rows() * m.state_elem() + history;
}

size_t Matcher::regions() const { return impl_->regions; }
void Matcher::set_origin(const Origin &origin) { impl_->origin = origin; }
Matcher::Origin Matcher::origin() const { return impl_->origin; }
int Matcher::device() const { return impl_->device; }
Status Matcher::poisoned() const { return impl_->poison; }
const std::vector<NeedleHipRun> &Matcher::run_list(size_t lane) const { return impl_->lanes[lane].runs; }
const uint32_t *Matcher::history(size_t lane) const { return impl_->lanes[lane].hist; }

}  // namespace needle
