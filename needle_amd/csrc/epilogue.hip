// The order-sensitive epilogue of a library job ON THE DEVICE: from the complete run list of all pairs to one
// SearchResult per video (needle/src/audio/comparator.rs:191-249 validity + BinaryHeap order, :405-515 find_best_match,
// :583-626 per-video walk), bit for bit what comparator.cpp computes on host threads.  At BASELINE.json configs[4]
// (2000 x 45 min: 3.95 M runs, ~3 950 candidates per video) the host form takes 68 ms on 16 threads -- and every rank of
// an 8-GPU job has a sixteenth of those threads -- while the work is 3e10 popcount-compares and a few small sorts.
//
//   bucket_count / scan / bucket_scatter : counting sort of the runs by problem (pair * regions + region)
//   pair_entries   : one thread per bucket -- the reference's reverse table walk order (src_end, then dst_end, descending),
//                    the duration validity tests (:212-223), std's BinaryHeap::push (append + sift up on the derived
//                    lexicographic Ord, :22-35) -> the bucket's entries in the heap's backing-array order (:249)
//   best_match     : one workgroup per video -- its pairs in lexicographic order, openings before endings inside a
//                    pair (:414-431) = the candidate numbering; links[k] = #{b : popcount(h_k ^ h_b) < bound} over ALL
//                    its candidates (:434-454): every pair, as int8 matrix products of the hashes' bits as +-1 whose
//                    sign bits are counted (exact: a dot product of +-1 bytes IS 32 - 2 popcount); score = -(links * 0.3f + secs * 0.7f) in unfused f32
//                    (:469); arg-min over (score, index) (:473-475); padding and hash duration (:479-481)
//
// Nothing here approximates: ties are broken by the candidate index exactly as the sorted (f32, usize) list of the
// reference breaks them.  tests: the GPU suite and tools/fuzz_pipeline.py with NEEDLE_HIP_DEVICE_EPILOGUE=1.
#include <map>
#include <mutex>

#include "epilogue.h"
#include "epilogue_kernels.h"

namespace needle {

namespace {

// A slab's runs into one block per destination rank (gpu_direct_runs).  A wave asks a block's counter once per destination
// for all its lanes' runs (a returning atomic per run on `world` addresses would be the kernel).
// How a run's pair becomes its two videos: the i-major numbering over n videos, or a library of seasons' grouped one
// (pair_ids.h; the tables in device memory: two bisections of global loads per run, over tables of a few KB -- this kernel
// runs once per job over the run list, not per cell).
struct DirectRowMajor {
  uint32_t n;
  __device__ void at(uint64_t p, uint32_t *i, uint32_t *j) const { pair_at_device(n, p, i, j); }
};
struct DirectGrouped {
  GroupView groups;
  // (every run of a grouped scan names a grouped pair; were one not to, it goes to video 0's owner and the epilogue drops it)
  __device__ void at(uint64_t p, uint32_t *i, uint32_t *j) const {
    if (!grouped_pair_at(groups, p, i, j)) *i = *j = 0;
  }
};
template <class Pairs>
__global__ __launch_bounds__(256) void direct_runs_kernel(const uint32_t *__restrict__ found, const NeedleHipRun *__restrict__ runs,
                                                          uint32_t slab_capacity, Pairs pairs, uint32_t regions, uint32_t videos_per_rank,
                                                          int world, uint8_t *__restrict__ send, DirectPlan plan) {
  const uint32_t total = min(*found, slab_capacity);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t base = blockIdx.x * blockDim.x; base < total; base += stride) {  // (whole waves stay in the loop: ballots)
    const uint32_t g = base + threadIdx.x;
    NeedleHipRun r{};
    uint32_t oi = 0xFFFFFFFFu, oj = 0xFFFFFFFFu;
    if (g < total) {
      r = runs[g];
      uint32_t vi, vj;
      pairs.at(r.problem / regions, &vi, &vj);
      oi = vi / videos_per_rank;
      oj = vj / videos_per_rank;
      if (oj == oi) oj = 0xFFFFFFFFu;
    }
    for (int q = 0; q < world; q++) {
      const bool mine = oi == (uint32_t)q || oj == (uint32_t)q;
      const unsigned long long mask = __builtin_amdgcn_ballot_w64(mine);
      if (mask == 0ull) continue;  // wave-uniform
      uint32_t *header = reinterpret_cast<uint32_t *>(send + plan.offset[q]);
      uint32_t first = 0u;
      if (lane == (uint32_t)(__ffsll((long long)mask) - 1)) first = atomicAdd(header, (uint32_t)__popcll(mask));
      first = (uint32_t)__shfl((int)first, __ffsll((long long)mask) - 1);
      if (mine) {
        const uint32_t at = first + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (at < plan.capacity[q]) reinterpret_cast<NeedleHipRun *>(send + plan.offset[q] + 32)[at] = r;
      }
    }
  }
}

struct EpilogueWorkspace {
  int device = 0;
  EntriesScratch scratch;
  DeviceBuffer<EpilogueControl> ctl;
  DeviceBuffer<uint32_t> links, row_len, row_ts;
  bool large_checked = false;
  bool large_ok = false;  // of the resident row tables: every row under 65 536 hashes, timestamps strictly increasing
  DeviceBuffer<uint64_t> row_seek, ts;
  // the grouped form's tables (pair_ids.h GroupView) and the videos' hash durations, and what they hold
  DeviceBuffer<uint32_t> group_of, rank_of, group_size, group_first, members;
  DeviceBuffer<uint64_t> group_base, hash_durations;
  std::vector<uint32_t> h_group_of, h_rank_of, h_group_size, h_group_first, h_members;
  std::vector<uint64_t> h_group_base, h_hash_durations;
  DeviceBuffer<DeviceEntry> entries;
  DeviceBuffer<Candidate> cand;
  DeviceBuffer<NeedleHipSearchResult> results;
  std::vector<uint32_t> h_row_len, h_row_ts;  // what the device tables hold
  std::vector<uint64_t> h_row_seek, h_ts;
};
std::mutex g_mu;
std::map<std::pair<int, int>, EpilogueWorkspace *> g_ws;  // (device, job slot)

EpilogueWorkspace *workspace(int slot) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(g_mu);
  EpilogueWorkspace *&w = g_ws[{dev, slot}];
  if (!w) {
    w = new EpilogueWorkspace();
    w->device = dev;
  }
  return w;
}

template <class T>
Status upload_if_changed(DeviceBuffer<T> *dst, std::vector<T> *resident, const std::vector<T> &want, hipStream_t stream) {
  if (dst->ptr && *resident == want) return Status::Ok();
  Status s = dst->reserve(std::max<size_t>(want.size(), 1));
  if (!s.ok()) return s;
  // (pageable source: the copy is staged by the runtime before the call returns)
  if (!want.empty()) NEEDLE_HIP_TRY(hipMemcpyAsync(dst->ptr, want.data(), want.size() * sizeof(T), hipMemcpyHostToDevice, stream));
  NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  *resident = want;
  return Status::Ok();
}

}  // namespace

std::atomic<uint64_t> &epilogue_host_fallbacks() {
  static std::atomic<uint64_t> count{0};
  return count;
}

void note_epilogue_host_fallback(const char *where, size_t runs, size_t videos) {
  epilogue_host_fallbacks().fetch_add(1);
  if (getenv("NEEDLE_HIP_TRACE"))
    std::fprintf(stderr, "[needle_hip] %s: a pair's bucket holds more than %u runs (silence / a sustained tone on both sides) or the rows are too long for the packed keys: the "
                         "per-video epilogue of this job (%zu runs, %zu videos) falls back to the HOST form\n",
                 where, kEpilogueLargeLimit, runs, videos);
}

Status gpu_direct_runs(const uint32_t *d_found, const NeedleHipRun *d_runs, uint32_t slab_capacity, uint32_t n, uint32_t regions,
                       uint32_t videos_per_rank, int world, uint8_t *d_send, const DirectPlan &plan, hipStream_t stream,
                       const GroupView *groups) {
  if (world < 1 || world > 64 || n < 2 || regions < 1 || videos_per_rank < 1)
    return Status::Make(NeedleError_InvalidArgument, "directed run exchange: invalid plan");
  for (int q = 0; q < world; q++) NEEDLE_HIP_TRY(hipMemsetAsync(d_send + plan.offset[q], 0, 32, stream));
  const uint32_t grid = (uint32_t)std::min<uint64_t>(2048, ((uint64_t)slab_capacity + 255) / 256);
  if (groups)
    hipLaunchKernelGGL(direct_runs_kernel<DirectGrouped>, dim3(std::max(grid, 1u)), dim3(256), 0, stream, d_found, d_runs, slab_capacity,
                       DirectGrouped{*groups}, regions, videos_per_rank, world, d_send, plan);
  else
    hipLaunchKernelGGL(direct_runs_kernel<DirectRowMajor>, dim3(std::max(grid, 1u)), dim3(256), 0, stream, d_found, d_runs, slab_capacity,
                       DirectRowMajor{n}, regions, videos_per_rank, world, d_send, plan);
  NEEDLE_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status gpu_epilogue_enqueue(const EpilogueJob &job, hipStream_t stream, NeedleHipSearchResult *host_results, uint32_t *host_failed) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());  // the per-device workspaces are shared, as everywhere else
  if (job.num_segments < 1 || job.num_segments > kMaxSegments)
    return Status::Make(NeedleError_InvalidArgument, "device epilogue: too many run segments");
  const GroupTables *groups = job.groups;
  if (groups && (!job.hash_durations || job.hash_durations->size() != job.n || groups->group_of.size() != job.n || groups->pairs() == 0))
    return Status::Make(NeedleError_InvalidArgument, "device epilogue: grouped job without pairs, or tables of another size");
  const uint64_t np = groups ? groups->pairs() : (uint64_t)job.n * (job.n - 1) / 2;
  const uint64_t buckets = np * job.regions;
  if (job.n < 2 || buckets >= 0xFFFFFFF0ull || job.max_runs >= 0xFFFFFFF0ull)
    return Status::Make(NeedleError_InvalidArgument, "device epilogue: library too large");
  EpilogueWorkspace *ws = workspace(job.slot);
  Status s;
  // what pair_entries_large_kernel's packed keys stand on, recomputed when the tables change (before they are taken over below):
  // every row under 65 536 hashes, every timestamp table strictly increasing (tables are shared by rows of equal length)
  if (!ws->large_checked || ws->h_ts != *job.ts || ws->h_row_len != *job.row_len || ws->h_row_ts != *job.row_ts) {
    static_assert(kEpilogueLargeLimit <= 8192, "13 bits of index in the packed key");
    bool ok = true;
    std::map<uint32_t, uint32_t> longest;  // table offset -> the longest row that reads it
    for (size_t r = 0; r < job.row_len->size() && ok; r++) {
      const uint32_t len = (*job.row_len)[r];
      ok = len < 65536u;
      uint32_t &m = longest[(*job.row_ts)[r]];
      m = std::max(m, len);
    }
    for (const auto &kv : longest) {
      const uint64_t *t = job.ts->data() + kv.first;
      for (uint32_t k = 1; k < kv.second && ok; k++) ok = t[k] > t[k - 1];
    }
    ws->large_ok = ok;
    ws->large_checked = true;
  }
  // row tables: only re-uploaded when the geometry changes
  if (!(s = upload_if_changed(&ws->row_len, &ws->h_row_len, *job.row_len, stream)).ok() ||
      !(s = upload_if_changed(&ws->row_ts, &ws->h_row_ts, *job.row_ts, stream)).ok() ||
      !(s = upload_if_changed(&ws->row_seek, &ws->h_row_seek, *job.row_seek, stream)).ok() ||
      !(s = upload_if_changed(&ws->ts, &ws->h_ts, *job.ts, stream)).ok())
    return s;
  GroupView view{};
  if (groups) {  // small, and the same from call to call while a library stands: re-uploaded when they change
    if (!(s = upload_if_changed(&ws->group_of, &ws->h_group_of, groups->group_of, stream)).ok() ||
        !(s = upload_if_changed(&ws->rank_of, &ws->h_rank_of, groups->rank_of, stream)).ok() ||
        !(s = upload_if_changed(&ws->group_size, &ws->h_group_size, groups->size, stream)).ok() ||
        !(s = upload_if_changed(&ws->group_first, &ws->h_group_first, groups->first, stream)).ok() ||
        !(s = upload_if_changed(&ws->members, &ws->h_members, groups->members, stream)).ok() ||
        !(s = upload_if_changed(&ws->group_base, &ws->h_group_base, groups->base, stream)).ok() ||
        !(s = upload_if_changed(&ws->hash_durations, &ws->h_hash_durations, *job.hash_durations, stream)).ok())
      return s;
    view = GroupView{ws->group_of.ptr, ws->rank_of.ptr, ws->group_size.ptr, ws->group_first.ptr, ws->group_base.ptr, ws->members.ptr,
                     (uint32_t)groups->size.size()};
  }
  const size_t runs = std::max<uint64_t>(job.max_runs, 1);
  if (!(s = ws->scratch.reserve(buckets, runs)).ok() || !(s = ws->entries.reserve(runs)).ok() || !(s = ws->cand.reserve(2 * runs)).ok() ||
      !(s = ws->links.reserve(2 * runs)).ok() || !(s = ws->ctl.reserve(1)).ok() || !(s = ws->results.reserve(job.n)).ok())
    return s;
  RunSegments segs;
  std::memset(&segs, 0, sizeof(segs));
  segs.count = job.num_segments;
  for (int k = 0; k < job.num_segments; k++) {
    segs.found[k] = job.segment_count[k];
    segs.runs[k] = job.segment_runs[k];
    segs.capacity[k] = job.segment_capacities[k] ? job.segment_capacities[k] : job.segment_capacity;
  }
  EpilogueParams pr = epilogue_params(job, ws->large_ok, job.n, buckets);
  pr.rows_per_video = job.rows_per_video;
  pr.v0 = job.v0;
  pr.v1 = job.v1;
  pr.hash_duration = job.hash_duration;
  if (groups && !job.block_wanted) {  // the comparator call, the index: every video
    pr.v0 = 0;
    pr.v1 = job.n;
  }
  if (pr.v0 > pr.v1 || pr.v1 > job.n) return Status::Make(NeedleError_InvalidArgument, "device epilogue: a block of videos outside the list");
  EpilogueControl *ctl = ws->ctl.ptr;
  NEEDLE_HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(*ctl), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(ws->results.ptr, 0, (size_t)job.n * sizeof(NeedleHipSearchResult), stream));
  if (!(s = enqueue_bucket_sort("epilogue_buckets", segs, pr.buckets, runs, &ws->scratch, stream)).ok()) return s;
  {
    KernelTimer timer("epilogue_entries", stream);
    s = groups ? enqueue_pair_entries<GroupedPairs>(ws->device, pr, ws->scratch, ws->row_len.ptr, ws->row_ts.ptr, ws->row_seek.ptr, ws->ts.ptr,
                                                    ws->entries.ptr, ctl, stream, view)
               : enqueue_pair_entries<RowMajorPairs>(ws->device, pr, ws->scratch, ws->row_len.ptr, ws->row_ts.ptr, ws->row_seek.ptr, ws->ts.ptr,
                                                     ws->entries.ptr, ctl, stream);
    if (!s.ok()) return s;
  }
  if (groups && pr.v1 > pr.v0) {  // workgroup b is video v0 + b
    KernelTimer timer("epilogue_best_match", stream);
    hipLaunchKernelGGL((best_match_kernel<GroupedVideos, GroupView, const uint64_t *>), dim3(pr.v1 - pr.v0), dim3(256), 0, stream, pr, ws->scratch.start.ptr,
                       ws->scratch.valid.ptr, ws->entries.ptr, ws->cand.ptr, &ctl->cand_cursor, ws->links.ptr, ws->results.ptr, &ctl->failed, view,
                       (const uint64_t *)ws->hash_durations.ptr);
  } else if (!groups && pr.v1 > pr.v0) {
    KernelTimer timer("epilogue_best_match", stream);
    hipLaunchKernelGGL(best_match_kernel<RowMajorVideos>, dim3(pr.v1 - pr.v0), dim3(256), 0, stream, pr, ws->scratch.start.ptr, ws->scratch.valid.ptr,
                       ws->entries.ptr, ws->cand.ptr, &ctl->cand_cursor, ws->links.ptr, ws->results.ptr, &ctl->failed);
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  NEEDLE_HIP_TRY(hipMemcpyAsync(host_results, ws->results.ptr, (size_t)job.n * sizeof(NeedleHipSearchResult), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(host_failed, &ctl->failed, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  return Status::Ok();
}

}  // namespace needle
