// Streaming comparator (include/needle_hip.h needle_hip_matcher_*): the search half of the streaming path.  S source
// sequences are resident in HBM; N lanes are destination sequences whose hashes arrive in chunks; a feed evaluates the
// cells of its new columns only and reports the runs those columns close, exactly the runs (and simhashes) that
// needle_hip_hamming_runs_host finds over the concatenation of a lane's chunks.
//
// State of a (lane, source): one run length per source row -- state[i] = length of the matching diagonal stretch that ends
// at cell (i, J - 1), J the lane's items so far (u16 where every source is shorter than 65 536 hashes, else u32) -- in
// two sets of buffers; and, per lane, its hashes so far (the destination simhash of a run reaches back over earlier chunks).
//
// One round (a feed, or a strip of one that is wider than kMaxStrip columns; also `finish` and `open`, with no columns):
//   land     matcher_land_kernel: the new chunks from the round's staging buffer to the end of their lanes' histories
//   scan     matcher_strip_kernel: a thread walks a diagonal of the strip (four, one after the other, of those that cross
//            column J - 1).  A diagonal that crosses column J - 1 starts from the carried length of the row it crosses it
//            at; one that enters through row 1 inside the strip starts at 0.  It walks its cells of the strip and reports a run where a cell breaks it or where it reaches the source's last
//            row; where it leaves through the strip's last column at row r it writes its length to row r of the OTHER set
//            (the state, shifted by the strip's width).  The set it reads is never written, so a round can be repeated.
//   simhash  matcher_simhash_kernel: both simhashes of every run reported, one wave per run (simhash_wave.h)
// Three launches whatever N and S: every kernel finds its lane in the round's lane table (blockIdx.y) and its source in
// the resident source table (through the resident list of every workgroup's source, blockIdx.x); only the lanes with data
// are in the grid.
#include "matcher.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "hipctx.h"
#include "simhash_wave.h"

namespace needle {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxStrip = 512;  // columns of one round per lane
constexpr uint32_t kCarriedRows = 1024;  // diagonals that cross column J - 1 per workgroup: four per thread, one after the other
// A source's workgroups: ceil((n - 1) / 1024) of diagonals that cross column J - 1 (the row they cross it at names them),
// then kTopBlocks of 256 diagonals that enter through row 1 at the strip's columns 1 .. W - 1.  The count is that of the
// widest strip, so the tables (sources, and the source of every workgroup) are built once; the workgroups a narrower strip
// does not need leave at once.
constexpr uint32_t kTopBlocks = (kMaxStrip - 1 + kThreads - 1) / kThreads;
constexpr uint32_t kEmitOpen = 1u;  // no state is written: the diagonals that reach the last column are reported (finish, open)
constexpr uint32_t kNoHash = 2u;    // the runs keep zero simhashes (open)
constexpr uint32_t kHeaderWords = 8;  // the slab: the run counter in word 0, the runs from byte 32
constexpr uint32_t kHeadRuns = 127;   // runs that come down with the counter in one copy

struct MatchSource {
  uint32_t src_off, n;  // arena offset and length (>= 2)
  uint32_t min_len, index;
  uint32_t row_off;     // of the source's rows inside a lane's state
  uint32_t block_base, carried_blocks, pad;
};

struct MatchLane {
  uint32_t *hist;    // the lane's hashes so far
  const void *from;  // state set the round reads ...
  void *to;          // ... and the one it writes
  uint32_t fed, width;      // J and the strip's columns [J, J + width)
  uint32_t stage_off;       // of the new hashes inside the round's buffer, in words
  uint32_t lane, flags, pad;
};
static_assert(sizeof(MatchLane) == 48, "lane table entries are 12 words");

struct MatchRun {  // NeedleHipRun + the lane (its slot in the round's table until the simhash kernel swaps the index in)
  uint32_t problem, src_end, dst_end, len, src_hash, dst_hash, lane, pad;
};

__global__ __launch_bounds__(kThreads) void matcher_land_kernel(const uint32_t *__restrict__ round_buf, uint32_t *__restrict__ count) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *count = 0u;
  const MatchLane ln = reinterpret_cast<const MatchLane *>(round_buf)[blockIdx.y];
  const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
  if (c < ln.width) ln.hist[ln.fed + c] = round_buf[ln.stage_off + c];
}

template <typename T>
__global__ __launch_bounds__(kThreads) void matcher_strip_kernel(const uint32_t *__restrict__ arena,
                                                                 const MatchSource *__restrict__ sources,
                                                                 const uint32_t *__restrict__ block_source,
                                                                 const MatchLane *__restrict__ lanes, uint32_t threshold,
                                                                 MatchRun *__restrict__ runs, uint32_t capacity,
                                                                 uint32_t *__restrict__ count) {
  __shared__ uint32_t strip[kMaxStrip];               // dst[J .. J + W)
  __shared__ uint32_t rows[kCarriedRows + kMaxStrip];  // the source rows this workgroup's diagonals meet
  const uint32_t lo = block_source[blockIdx.x];
  const MatchSource sc = sources[lo];
  const MatchLane ln = lanes[blockIdx.y];
  const uint32_t n = sc.n, W = ln.width, J = ln.fed, tid = threadIdx.x;
  const uint32_t b = blockIdx.x - sc.block_base;
  const bool carried = b < sc.carried_blocks;
  // carried: the diagonals that cross column J - 1 at rows b * kCarriedRows ..; otherwise those that enter through row 1 at
  // the strip's columns q0 ..
  const uint32_t q0 = carried ? 0u : (b - sc.carried_blocks) * kThreads + 1u;
  if (!carried && q0 >= W) return;  // (the whole workgroup)
  const uint32_t seg0 = carried ? b * kCarriedRows + 1u : 1u;  // first row staged
  const uint32_t steps = W - q0;                               // the most cells one of the workgroup's diagonals walks
  {
    const uint32_t seg_rows = steps ? min(n - seg0, (carried ? kCarriedRows : kThreads) - 1u + steps) : 0u;  // rows seg0 .. <= n - 1
    const uint32_t *__restrict__ src = arena + sc.src_off + seg0;
    for (uint32_t k = tid; k < seg_rows; k += kThreads) rows[k] = src[k];
    for (uint32_t k = tid; k < W; k += kThreads) strip[k] = ln.hist[J + k];
  }
  __syncthreads();

  const uint32_t lane = tid & 63u;
  const uint32_t min_len = sc.min_len;
  const bool emit_open = (ln.flags & kEmitOpen) != 0u;
  // The runs of one step leave the wave together: one returning atomic for all of them (search.hip, round 6).
  auto push = [&](const bool want, const uint32_t src_end, const uint32_t dst_end, const uint32_t len) {
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(want);
    if (mask == 0ull) return;
    uint32_t base = 0u;
    if (lane == 0u) base = atomicAdd(count, (uint32_t)__popcll(mask));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (want && slot < capacity) runs[slot] = MatchRun{lo, src_end, dst_end, len, 0u, 0u, blockIdx.y, 0u};
  };
  // One diagonal per thread: first new cell (i0, J + q), `rel` = i0's place in the staged rows, `run` = the carried length.
  // It walks w cells (i0 + c, J + q + c).  Every thread of the workgroup comes through here together.
  auto walk = [&](const bool live, const uint32_t i0, const uint32_t q, const uint32_t rel, uint32_t run) {
    const uint32_t w = live ? min(W - q, n - i0) : 0u;
    for (uint32_t c = 0; c < steps; c++) {
      bool ended = false;
      uint32_t len = 0u;
      if (c < w) {
        // column 0 is no cell
        const bool match = J + q + c >= 1u && (uint32_t)__popc(rows[rel + c] ^ strip[q + c]) <= threshold;
        ended = !match && run >= min_len;  // the run ended at the previous cell
        len = run;
        run = match ? run + 1u : 0u;
      }
      push(ended, i0 + c - 1u, J + q + c - 1u, len);
    }
    // the last cell walked (with no columns: the cell of the carried length itself)
    const uint32_t r = i0 + w - 1u, j = J + q + w - 1u;
    const bool last_row = live && w > 0u && r == n - 1u;
    const bool last_col = live && !last_row;  // then q + w == W
    push((last_row || (last_col && emit_open)) && run >= min_len, r, j, run);
    if (last_col && !emit_open) (static_cast<T *>(ln.to) + sc.row_off)[r] = (T)run;
  };
  if (carried) {
    for (uint32_t part = 0; part < kCarriedRows; part += kThreads) {
      const uint32_t t = b * kCarriedRows + part + tid;  // crosses column J - 1 at row t (row 0 is no cell: its length is 0)
      if (t - tid >= n - 1u) break;                      // (the whole workgroup)
      const bool live = t < n - 1u;
      const uint32_t run = live && J > 0u && t >= 1u ? (uint32_t)(static_cast<const T *>(ln.from) + sc.row_off)[t] : 0u;
      walk(live, t + 1u, 0u, part + tid, run);
    }
  } else {
    const uint32_t q = q0 + tid;  // enters through row 1 at column J + q
    walk(q < W, 1u, q, 0u, 0u);
  }
}

__global__ __launch_bounds__(kThreads) void matcher_simhash_kernel(const uint32_t *__restrict__ arena,
                                                                   const MatchSource *__restrict__ sources,
                                                                   const MatchLane *__restrict__ lanes,
                                                                   MatchRun *__restrict__ runs, uint32_t capacity,
                                                                   const uint32_t *__restrict__ count) {
  const uint32_t total = min(*count, capacity);
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  const TransposeLane t = transpose_lane(lane);
  for (uint32_t k = wave; k < total; k += waves) {
    const MatchRun r = runs[k];
    const MatchSource sc = sources[r.problem];
    const MatchLane ln = lanes[r.lane];
    uint32_t src_hash = 0u, dst_hash = 0u;
    if ((ln.flags & kNoHash) == 0u) {  // (wave-uniform)
      src_hash = wave_simhash32(arena + sc.src_off + (r.src_end - r.len), r.len + 1u, lane, t);
      dst_hash = wave_simhash32(ln.hist + (r.dst_end - r.len), r.len + 1u, lane, t);
    }
    if (lane == 0) {
      runs[k].problem = sc.index;
      runs[k].lane = ln.lane;
      runs[k].src_hash = src_hash;
      runs[k].dst_hash = dst_hash;
    }
  }
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
  uint32_t threshold = 0;
  bool narrow = true;       // u16 run lengths
  uint64_t total_rows = 0;  // of one lane's state
  uint64_t cells_per_column = 0;  // sum of n_s - 1
  uint32_t total_blocks = 0;
  std::vector<MatchSource> table;
  std::vector<LaneState> lanes;
  DeviceBuffer<uint32_t> arena;
  DeviceBuffer<MatchSource> d_table;
  std::vector<uint32_t> block_source;  // the table entry of every workgroup of the scan's grid
  DeviceBuffer<uint32_t> d_block_source;
  DeviceBuffer<uint8_t> state[2];
  DeviceBuffer<uint32_t> d_round, slab;
  uint32_t capacity = 4096;  // runs the slab holds
  PinnedStage round_stage, head_stage;
  Status poison = Status::Ok();
  uint64_t feeds = 0, launches = 0, cells = 0, arena_bytes = 0;

  ~Impl() {
    std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
    for (LaneState &l : lanes)
      if (l.hist) (void)hipFree(l.hist);
    for (PinnedStage *st : {&round_stage, &head_stage}) {
      if (st->ptr) (void)hipHostFree(st->ptr);
      if (st->done) (void)hipEventDestroy(st->done);
    }
  }

  size_t state_elem() const { return narrow ? sizeof(uint16_t) : sizeof(uint32_t); }

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
    for (size_t a = 0; a < k; a++) {
      const Piece &p = pieces[a];
      const LaneState &l = lanes[p.lane];
      MatchLane &e = lt[a];
      e.hist = l.hist;
      e.from = state[l.cur].ptr + (uint64_t)p.lane * total_rows * state_elem();
      e.to = state[l.cur ^ 1].ptr + (uint64_t)p.lane * total_rows * state_elem();
      e.fed = (uint32_t)l.fed;
      e.width = p.width;
      e.stage_off = (uint32_t)words;
      e.lane = (uint32_t)p.lane;
      e.flags = p.flags;
      e.pad = 0;
      words += p.width;
      round_cells += cells_per_column * (uint64_t)(p.width - (l.fed == 0 && p.width ? 1u : 0u));
    }
    if (!(s = d_round.reserve(words)).ok() || !(s = round_stage.acquire(words * 4)).ok()) return s;
    std::memcpy(round_stage.ptr, lt.data(), k * sizeof(MatchLane));
    for (size_t a = 0; a < k; a++)
      if (pieces[a].width) std::memcpy(static_cast<uint32_t *>(round_stage.ptr) + lt[a].stage_off, pieces[a].items, (size_t)pieces[a].width * 4);
    NEEDLE_HIP_TRY(hipMemcpyAsync(d_round.ptr, round_stage.ptr, words * 4, hipMemcpyHostToDevice, stream));
    round_stage.mark(stream);

    const MatchLane *d_lanes = reinterpret_cast<const MatchLane *>(d_round.ptr);
    const dim3 block(kThreads);
    std::vector<MatchRun> got;
    for (;;) {
      if (!(s = slab.reserve(kHeaderWords + (uint64_t)capacity * (sizeof(MatchRun) / 4))).ok()) return s;
      uint32_t *d_count = slab.ptr;
      MatchRun *d_runs = reinterpret_cast<MatchRun *>(slab.ptr + kHeaderWords);
      {
        KernelTimer timer("matcher_land");
        hipLaunchKernelGGL(matcher_land_kernel, dim3((std::max(widest, 1u) + kThreads - 1) / kThreads, (uint32_t)k), block, 0, stream,
                           d_round.ptr, d_count);
        NEEDLE_HIP_TRY(hipGetLastError());
      }
      {
        KernelTimer timer("matcher_strip");
        if (narrow)
          hipLaunchKernelGGL(matcher_strip_kernel<uint16_t>, dim3(total_blocks, (uint32_t)k), block, 0, stream, arena.ptr, d_table.ptr,
                             d_block_source.ptr, d_lanes, threshold, d_runs, capacity, d_count);
        else
          hipLaunchKernelGGL(matcher_strip_kernel<uint32_t>, dim3(total_blocks, (uint32_t)k), block, 0, stream, arena.ptr, d_table.ptr,
                             d_block_source.ptr, d_lanes, threshold, d_runs, capacity, d_count);
        NEEDLE_HIP_TRY(hipGetLastError());
      }
      {
        KernelTimer timer("matcher_simhash");
        hipLaunchKernelGGL(matcher_simhash_kernel, dim3((uint32_t)device_cu_count() * 2u), block, 0, stream, arena.ptr, d_table.ptr, d_lanes,
                           d_runs, capacity, d_count);
        NEEDLE_HIP_TRY(hipGetLastError());
      }
      launches += 3;
      cells += round_cells;
      // the counter and the first runs in one copy; the rest, if any, in a second one
      const uint32_t head = std::min(capacity, kHeadRuns);
      const size_t head_bytes = kHeaderWords * 4 + (size_t)head * sizeof(MatchRun);
      if (!(s = head_stage.acquire(head_bytes)).ok()) return s;
      NEEDLE_HIP_TRY(hipMemcpyAsync(head_stage.ptr, slab.ptr, head_bytes, hipMemcpyDeviceToHost, stream));
      NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
      round_stage.pending = false;
      const uint32_t found = *static_cast<const uint32_t *>(head_stage.ptr);
      if (found > capacity) {  // nothing is lost: a larger slab, and the round again from the set it did not write
        capacity = std::max(found, capacity * 2);
        continue;
      }
      got.resize(found);
      const uint32_t first = std::min(found, head);
      if (first) std::memcpy(got.data(), static_cast<const char *>(head_stage.ptr) + kHeaderWords * 4, (size_t)first * sizeof(MatchRun));
      if (found > first) NEEDLE_HIP_TRY(hipMemcpy(got.data() + first, d_runs + first, (size_t)(found - first) * sizeof(MatchRun), hipMemcpyDeviceToHost));
      break;
    }
    for (const MatchRun &r : got) {
      const NeedleHipRun out{r.problem, r.src_end, r.dst_end, r.len, r.src_hash, r.dst_hash};
      if (open_out) open_out->push_back(out);
      else lanes[r.lane].runs.push_back(out);
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
    Status s = round(pieces, open_out);
    if (!s.ok() && s.code != NeedleError_InvalidArgument && s.code != NeedleError_NullArgument) poison = s;
    return s;
  }
};

Matcher::Matcher() : impl_(new Impl()) {}
Matcher::~Matcher() = default;
size_t Matcher::lanes() const { return impl_->n; }

Status Matcher::Create(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len,
                       size_t num_sources, size_t lanes, uint32_t threshold, std::unique_ptr<Matcher> *out) {
  if (!sources || !min_len || !out || (num_hashes && !hashes)) return Status::Make(NeedleError_NullArgument, "matcher: null argument");
  if (lanes == 0 || lanes > 65535) return Status::Make(NeedleError_InvalidArgument, "matcher: lanes must be 1 to 65535");
  if (num_sources == 0 || num_sources > 0xFFFFFFFFull || num_hashes > 0xFFFFFFFFull)
    return Status::Make(NeedleError_InvalidArgument, "matcher: 1 to 2^32 - 1 sources inside at most 2^32 - 1 hashes");
  std::unique_ptr<Matcher> mt(new Matcher());
  Impl &m = *mt->impl_;
  uint64_t blocks = 0;
  for (size_t s = 0; s < num_sources; s++) {
    if (min_len[s] == 0) return Status::Make(NeedleError_InvalidArgument, "matcher: min_len must be >= 1");
    if ((uint64_t)sources[s].offset + sources[s].len > num_hashes) return Status::Make(NeedleError_InvalidArgument, "matcher: a source lies outside the hashes");
    const uint32_t len = sources[s].len;
    if (len >= 65536) m.narrow = false;
    if (len >= 2) {  // a shorter source has no cells
      MatchSource e{};
      e.src_off = sources[s].offset;
      e.n = len;
      e.min_len = min_len[s];
      e.index = (uint32_t)s;
      e.row_off = (uint32_t)m.total_rows;
      e.block_base = (uint32_t)blocks;
      e.carried_blocks = (len - 1 + kCarriedRows - 1) / kCarriedRows;
      blocks += e.carried_blocks + kTopBlocks;
      m.total_rows += len;
      m.cells_per_column += len - 1;
      m.block_source.insert(m.block_source.end(), e.carried_blocks + kTopBlocks, (uint32_t)m.table.size());
      m.table.push_back(e);
    }
    if (blocks > 0x7FFFFFFFull || m.total_rows > 0xFFFFFFFFull) return Status::Make(NeedleError_InvalidArgument, "matcher: the sources are too long together");
  }
  m.n = lanes;
  m.threshold = threshold;
  m.total_blocks = (uint32_t)blocks;
  m.lanes = std::vector<LaneState>(lanes);
  if (const char *e = getenv("NEEDLE_HIP_MATCHER_RUN_SLAB")) m.capacity = (uint32_t)std::min<long long>(std::max(1ll, atoll(e)), 1ll << 26);

  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = ensure_device();
  if (!s.ok()) return s;
  if (!m.table.empty()) {
    hipStream_t stream = library_stream();
    const uint64_t state_bytes = (uint64_t)lanes * m.total_rows * m.state_elem();
    if (!(s = m.arena.reserve(std::max<size_t>(num_hashes, 1))).ok() || !(s = m.d_table.reserve(m.table.size())).ok() ||
        !(s = m.d_block_source.reserve(m.block_source.size())).ok() ||
        !(s = m.state[0].reserve(state_bytes)).ok() || !(s = m.state[1].reserve(state_bytes)).ok())
      return s;
    m.arena_bytes = num_hashes * sizeof(uint32_t);
    NEEDLE_HIP_TRY(hipMemcpyAsync(m.arena.ptr, hashes, num_hashes * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    NEEDLE_HIP_TRY(hipMemcpyAsync(m.d_table.ptr, m.table.data(), m.table.size() * sizeof(MatchSource), hipMemcpyHostToDevice, stream));
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
        if (m.table.empty()) {  // no source has a cell: the lane only counts
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
  if (!feeder) return Status::Make(NeedleError_NullArgument, "matcher: null argument");
  if (feeder->lanes() != m.n) return Status::Make(NeedleError_InvalidArgument, "matcher: the feeder has another number of lanes");
  if (!m.poison.ok()) return m.poison;
  std::vector<std::vector<uint32_t>> taken(m.n);
  std::vector<const uint32_t *> ptrs(m.n, nullptr);
  std::vector<size_t> counts(m.n, 0), finish;
  for (size_t i = 0; i < m.n; i++) {
    size_t kept = 0;
    bool finished = false;
    Status s = feeder->Ready(i, &kept, nullptr, &finished);
    if (!s.ok()) return s;
    const LaneState &l = m.lanes[i];
    if (l.finished) {
      if (kept != l.fed || !finished) return Status::Make(NeedleError_InvalidArgument, "matcher: the lane is finished (reset it first)");
      continue;
    }
    if (kept < l.fed) return Status::Make(NeedleError_InvalidArgument, "matcher: the feeder's lane holds fewer items than the matcher has taken");
    taken[i].resize(kept - l.fed);
    if (!taken[i].empty() && !(s = feeder->Items(i, (size_t)l.fed, taken[i].size(), taken[i].data())).ok()) return s;
    ptrs[i] = taken[i].data();
    counts[i] = taken[i].size();
    if (finished) finish.push_back(i);
  }
  Status s = Feed(ptrs.data(), counts.data());
  if (!s.ok() || finish.empty()) return s;
  return Finish(finish.data(), finish.size());
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
  if (pieces.empty()) return Status::Ok();
  if (m.table.empty()) {
    for (const Piece &p : pieces) m.lanes[p.lane].finished = true;
    return Status::Ok();
  }
  return m.guarded_round(pieces, nullptr);
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
  if (m.lanes[lane].finished || m.lanes[lane].fed == 0 || m.table.empty()) return Status::Ok();  // nothing is open
  return m.guarded_round({Piece{lane, nullptr, 0u, kEmitOpen | kNoHash}}, runs);
}

void Matcher::Stats(uint64_t stats[4]) const {
  const Impl &m = *impl_;
  uint64_t history = 0;
  for (const LaneState &l : m.lanes) history += l.fed * sizeof(uint32_t);
  stats[0] = m.feeds;
  stats[1] = m.launches;
  stats[2] = m.cells;
  stats[3] = m.arena_bytes + 2 * (uint64_t)m.n * m.total_rows * m.state_elem() + history;
}

}  // namespace needle
