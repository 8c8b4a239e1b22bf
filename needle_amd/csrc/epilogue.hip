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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>

#include "../../include/needle_hip.h"
#include "epilogue.h"
#include "hipctx.h"

namespace needle {

namespace {

constexpr int kMaxSegments = 64;

struct RunSegments {  // the run list in pieces: a device word with the runs found, and the runs
  const uint32_t *found[kMaxSegments];
  const NeedleHipRun *runs[kMaxSegments];
  uint32_t capacity[kMaxSegments];
  int count;
};

struct DeviceEntry {  // ComparatorHeapEntry (:22-35) without the fields that are constant inside a bucket
  uint64_t src_start, src_end, dst_start, dst_end;
  uint32_t score, src_hash, dst_hash, pad;
};

struct Candidate {  // :410-432
  uint64_t start, end;
  uint32_t hash, is_opening;
};

struct EpilogueParams {
  uint32_t n, regions, buckets;          // videos, comparator regions, np * regions
  uint32_t large_ok;                     // buckets beyond kEpilogueBucketLimit may go to pair_entries_large_kernel (see there)
  uint32_t rows_per_video;               // rows of the hash arena per video
  uint32_t v0, v1;                       // the videos whose results are wanted
  uint32_t bound;                        // threshold + threshold / 2 (:441)
  uint32_t include_endings;
  uint64_t min_duration[2];              // [0] opening, [1] ending
  uint64_t time_padding, hash_duration;
};

__device__ __forceinline__ uint32_t segment_count(const RunSegments &s, int k) {
  return min(*s.found[k], s.capacity[k]);  // an overflowed slab is redone by the host
}

// run g of the concatenated list (segments in rank order)
__device__ __forceinline__ bool locate_run(const RunSegments &s, uint64_t g, NeedleHipRun *out) {
  for (int k = 0; k < s.count; k++) {
    const uint32_t c = segment_count(s, k);
    if (g < c) {
      *out = s.runs[k][g];
      return true;
    }
    g -= c;
  }
  return false;
}

__global__ __launch_bounds__(256) void bucket_count_kernel(RunSegments segs, uint32_t buckets, uint32_t *__restrict__ count) {
  uint64_t total = 0;
  for (int k = 0; k < segs.count; k++) total += segment_count(segs, k);
  for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g < total; g += (uint64_t)gridDim.x * blockDim.x) {
    NeedleHipRun r;
    if (locate_run(segs, g, &r) && r.problem < buckets) atomicAdd(&count[r.problem], 1u);
  }
}

// exclusive scan of count[0..n) into start[0..n], start[n] = total: per-block sums, one block over them, then the blocks
constexpr int kScanBlock = 1024;
__global__ __launch_bounds__(256) void scan_block_sums_kernel(const uint32_t *__restrict__ count, uint32_t n, uint32_t *__restrict__ sums) {
  __shared__ uint32_t part[256];
  const uint32_t base = blockIdx.x * kScanBlock;
  uint32_t s = 0;
  for (int k = 0; k < 4; k++) {
    const uint32_t i = base + threadIdx.x * 4 + k;
    s += i < n ? count[i] : 0u;
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}
__global__ __launch_bounds__(256) void scan_sums_kernel(uint32_t *__restrict__ sums, uint32_t blocks) {  // one workgroup
  __shared__ uint32_t carry;
  __shared__ uint32_t part[256];
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < blocks; base += 256) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < blocks ? sums[i] : 0u;
    part[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // inclusive Hillis-Steele
      const uint32_t add = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
      __syncthreads();
      part[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < blocks) sums[i] = carry + part[threadIdx.x] - v;  // exclusive
    __syncthreads();
    if (threadIdx.x == 255) carry += part[255];
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void scan_apply_kernel(const uint32_t *__restrict__ count, uint32_t n, const uint32_t *__restrict__ sums,
                                                         uint32_t *__restrict__ start) {
  __shared__ uint32_t part[256];
  const uint32_t base = blockIdx.x * kScanBlock;
  uint32_t v[4], s = 0;
  for (int k = 0; k < 4; k++) {
    const uint32_t i = base + threadIdx.x * 4 + k;
    v[k] = i < n ? count[i] : 0u;
    s += v[k];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const uint32_t add = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t run = sums[blockIdx.x] + part[threadIdx.x] - s;
  for (int k = 0; k < 4; k++) {
    const uint32_t i = base + threadIdx.x * 4 + k;
    if (i < n) start[i] = run;
    run += v[k];
    if (i + 1 == n) start[n] = run;
  }
}

__global__ __launch_bounds__(256) void bucket_scatter_kernel(RunSegments segs, uint32_t buckets, const uint32_t *__restrict__ start,
                                                             uint32_t *__restrict__ fill, NeedleHipRun *__restrict__ sorted) {
  uint64_t total = 0;
  for (int k = 0; k < segs.count; k++) total += segment_count(segs, k);
  for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g < total; g += (uint64_t)gridDim.x * blockDim.x) {
    NeedleHipRun r;
    if (locate_run(segs, g, &r) && r.problem < buckets) sorted[start[r.problem] + atomicAdd(&fill[r.problem], 1u)] = r;
  }
}

// pairs (i, j), i < j, i-major (comparator.rs:534-545): the inverse of the numbering, exact (hostutil's pair_at)
__device__ __forceinline__ uint64_t row_start(uint64_t n, uint64_t i) { return i * (2 * n - i - 1) / 2; }
__device__ __forceinline__ void pair_at_device(uint64_t n, uint64_t index, uint32_t *pi, uint32_t *pj) {
  const double b = 2.0 * (double)n - 1.0;
  const double disc = b * b - 8.0 * (double)index;
  uint64_t i = disc > 0.0 ? (uint64_t)((b - sqrt(disc)) / 2.0) : 0;
  if (i + 2 > n) i = n >= 2 ? n - 2 : 0;
  while (i > 0 && row_start(n, i) > index) i--;
  while (i + 2 < n && row_start(n, i + 1) <= index) i++;
  *pi = (uint32_t)i;
  *pj = (uint32_t)(i + 1 + (index - row_start(n, i)));
}

// pairs (i, j), i < j, j-major: p(i, j) = j (j - 1) / 2 + i (the incremental index's store, index.cpp): an id does not depend
// on the number of videos, so appending videos only adds ids at the end.  The inverse, exact like pair_at_device.
__device__ __forceinline__ uint64_t column_start(uint64_t j) { return j * (j - 1) / 2; }
__device__ __forceinline__ void column_pair_at(uint64_t index, uint32_t *pi, uint32_t *pj) {
  uint64_t j = (uint64_t)((1.0 + sqrt(1.0 + 8.0 * (double)index)) / 2.0);
  if (j < 1) j = 1;
  while (j > 1 && column_start(j) > index) j--;
  while (column_start(j + 1) <= index) j++;
  *pi = (uint32_t)(index - column_start(j));
  *pj = (uint32_t)j;
}

// How pair_entries_kernel / pair_entries_large_kernel turn a bucket's pair into its two videos.  Built in the kernel from
// EpilogueParams and the kernel's trailing arguments (none for the library job's form: its code is what it was).
struct RowMajorPairs {  // NeedleHipRun.problem / regions = the pair's index in the reference's i-major list over pr.n videos
  uint64_t n;
  __device__ explicit RowMajorPairs(const EpilogueParams &pr) : n(pr.n) {}
  __device__ void at(uint64_t p, uint32_t *i, uint32_t *j) const { pair_at_device(n, p, i, j); }
};
struct ColumnMajorPairs {  // an index append: problem / regions = p(i, j) - first, first = the append's first new pair
  uint64_t first;
  __device__ ColumnMajorPairs(const EpilogueParams &, uint64_t first_pair) : first(first_pair) {}
  __device__ void at(uint64_t p, uint32_t *i, uint32_t *j) const { column_pair_at(first + p, i, j); }
};
struct ListedPairs {  // an index edit: problem / regions = a listed pair, table[listed] = its id p(i, j) in the rebuilt store
  const uint32_t *table;
  __device__ ListedPairs(const EpilogueParams &, const uint32_t *pair_ids) : table(pair_ids) {}
  __device__ void at(uint64_t p, uint32_t *i, uint32_t *j) const { column_pair_at(table[p], i, j); }
};

// A slab's runs into one block per destination rank (gpu_direct_runs).  A wave asks a block's counter once per destination
// for all its lanes' runs (a returning atomic per run on `world` addresses would be the kernel).
__global__ __launch_bounds__(256) void direct_runs_kernel(const uint32_t *__restrict__ found, const NeedleHipRun *__restrict__ runs,
                                                          uint32_t slab_capacity, uint32_t n, uint32_t regions, uint32_t videos_per_rank,
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
      pair_at_device(n, r.problem / regions, &vi, &vj);
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

// #[derive(Ord)] over (score, src_start, src_end, dst_start, dst_end, src_match_hash, dst_match_hash, ...): the rest of
// the fields are equal for all entries of one bucket.  true: a > b.
__device__ __forceinline__ bool entry_greater(const DeviceEntry &a, const DeviceEntry &b) {
  if (a.score != b.score) return a.score > b.score;
  if (a.src_start != b.src_start) return a.src_start > b.src_start;
  if (a.src_end != b.src_end) return a.src_end > b.src_end;
  if (a.dst_start != b.dst_start) return a.dst_start > b.dst_start;
  if (a.dst_end != b.dst_end) return a.dst_end > b.dst_end;
  if (a.src_hash != b.src_hash) return a.src_hash > b.src_hash;
  return a.dst_hash > b.dst_hash;
}

// One thread per bucket.  row tables: length, offset of the row's timestamps in `ts` (un-seeked, shared by rows of equal
// length), seek added to every timestamp of the row.
template <class Pairs, class... Extra>
__global__ __launch_bounds__(64) void pair_entries_kernel(EpilogueParams pr, const uint32_t *__restrict__ start,
                                                          NeedleHipRun *__restrict__ sorted, const uint32_t *__restrict__ row_len,
                                                          const uint32_t *__restrict__ row_ts, const uint64_t *__restrict__ row_seek,
                                                          const uint64_t *__restrict__ ts, DeviceEntry *__restrict__ entries,
                                                          uint32_t *__restrict__ valid, uint32_t *__restrict__ failed,
                                                          uint32_t *__restrict__ large_count, uint32_t *__restrict__ large_list, Extra... extra) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= pr.buckets) return;
  const uint32_t lo = start[b], hi = start[b + 1];
  uint32_t out = 0;
  if (hi - lo > kEpilogueBucketLimit) {
    // One lane orders a bucket by insertion (quadratic) and builds its heap alone: right for the handful of runs a pair of
    // episodes has, not for the hundreds two stretches of silence or of one sustained tone produce (an S x S block of equal
    // hashes is ~2 S runs).  Such a bucket goes on the list of pair_entries_large_kernel (a workgroup each; the list cannot
    // overflow: every entry stands for more than kEpilogueBucketLimit of the runs it was sized by); beyond what that kernel
    // holds in LDS the library is handed back to the host form (threaded, n log n): bit 31 of `failed`.
    if (pr.large_ok && hi - lo <= kEpilogueLargeLimit) large_list[atomicAdd(large_count, 1u)] = b;
    else atomicOr(failed, kEpilogueBucketTooLarge);
    return;  // (valid[b]: the large kernel's)
  } else if (hi > lo) {
    // the reference walks its table backwards: i = n-1..1 and, inside, j = m-1..1 (:191-192)
    for (uint32_t a = lo + 1; a < hi; a++) {
      const NeedleHipRun x = sorted[a];
      uint32_t q = a;
      while (q > lo) {
        const NeedleHipRun y = sorted[q - 1];
        const bool before = y.src_end != x.src_end ? y.src_end > x.src_end : y.dst_end > x.dst_end;
        if (before) break;
        sorted[q] = y;
        q--;
      }
      sorted[q] = x;
    }
    const uint32_t region = b % pr.regions;
    uint32_t vi, vj;
    Pairs(pr, extra...).at(b / pr.regions, &vi, &vj);
    const uint32_t src_row = vi * pr.rows_per_video + region, dst_row = vj * pr.rows_per_video + region;
    const uint32_t src_len = row_len[src_row], dst_len = row_len[dst_row];
    const uint64_t *src_ts = ts + row_ts[src_row], *dst_ts = ts + row_ts[dst_row];
    const uint64_t src_seek = row_seek[src_row], dst_seek = row_seek[dst_row];
    const uint64_t min_duration = pr.min_duration[region];
    DeviceEntry *heap = entries + lo;
    for (uint32_t a = lo; a < hi; a++) {
      const NeedleHipRun r = sorted[a];
      const uint32_t i = r.src_end, j = r.dst_end, len = r.len;
      if (len == 0 || len > i || len > j || i >= src_len || j >= dst_len) continue;
      DeviceEntry e;
      e.src_start = src_ts[i - len] + src_seek;  // one BEFORE the first matched cell (:206-207)
      e.src_end = src_ts[i] + src_seek;
      e.dst_start = dst_ts[j - len] + dst_seek;
      e.dst_end = dst_ts[j] + dst_seek;
      if (e.src_end < e.src_start || e.dst_end < e.dst_start) continue;
      if (e.src_end - e.src_start < min_duration || e.dst_end - e.dst_start < min_duration) continue;  // :212-223
      e.score = len;
      e.src_hash = r.src_match_hash;
      e.dst_hash = r.dst_match_hash;
      e.pad = 0;
      // BinaryHeap::push: append, sift up while greater than the parent
      uint32_t pos = out++;
      while (pos > 0) {
        const uint32_t parent = (pos - 1) / 2;
        const DeviceEntry p = heap[parent];
        if (!entry_greater(e, p)) break;
        heap[pos] = p;
        pos = parent;
      }
      heap[pos] = e;
    }
  }
  valid[b] = out;
}

// One WORKGROUP per bucket of more than kEpilogueBucketLimit runs (round 6; the hostile corpus: silence against silence).
// The same three steps as the lane above, on packed keys in LDS (8 bytes per run):
//   1. walk order: bitonic sort by (src_end, dst_end) descending -- key (0xFFFF - src_end) << 16 | (0xFFFF - dst_end), the
//      run's index in the low word;
//   2. every thread turns its sorted elements into (rank << 16 | valid << 15 | index): rank = len << 32 | (src_end - len) << 16
//      | dst_end IS the derived Ord of :22-35 inside one bucket -- score = len, and with timestamps that strictly increase along
//      a row (checked on the host: large_ok) src_start / src_end / dst_start / dst_end order as src_end - len, src_end,
//      dst_end - len, dst_end; two runs of a bucket never share (src_end, dst_end), so the hashes are never reached;
//   3. ONE lane replays BinaryHeap::push over the valid elements in walk order, in place (the heap never holds more than the
//      elements already consumed); then every thread builds the DeviceEntry of its heap slots.
template <class Pairs, class... Extra>
__global__ __launch_bounds__(256) void pair_entries_large_kernel(EpilogueParams pr, const uint32_t *__restrict__ start,
                                                                 const NeedleHipRun *__restrict__ sorted, const uint32_t *__restrict__ row_len,
                                                                 const uint32_t *__restrict__ row_ts, const uint64_t *__restrict__ row_seek,
                                                                 const uint64_t *__restrict__ ts, DeviceEntry *__restrict__ entries,
                                                                 uint32_t *__restrict__ valid, const uint32_t *__restrict__ large_count,
                                                                 const uint32_t *__restrict__ large_list, Extra... extra) {
  extern __shared__ unsigned long long arr[];  // kEpilogueLargeLimit elements
  __shared__ uint32_t heap_size;
  const uint32_t t = threadIdx.x;
  const uint32_t listed = *large_count;
  for (uint32_t item = blockIdx.x; item < listed; item += gridDim.x) {
    const uint32_t b = large_list[item];
    const uint32_t lo = start[b], n = start[b + 1] - lo;
    uint32_t p2 = 1;
    while (p2 < n) p2 <<= 1;
    for (uint32_t a = t; a < p2; a += 256) {
      unsigned long long v = ~0ull;
      if (a < n) {
        const NeedleHipRun r = sorted[lo + a];
        v = ((unsigned long long)(((0xFFFFu - (r.src_end & 0xFFFFu)) << 16) | (0xFFFFu - (r.dst_end & 0xFFFFu))) << 32) | a;
      }
      arr[a] = v;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= p2; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t a = t; a < p2; a += 256) {
          const uint32_t partner = a ^ j;
          if (partner > a) {
            const unsigned long long x = arr[a], y = arr[partner];
            const bool up = (a & k) == 0;
            if ((x > y) == up) {
              arr[a] = y;
              arr[partner] = x;
            }
          }
        }
        __syncthreads();
      }
    const uint32_t region = b % pr.regions;
    uint32_t vi, vj;
    Pairs(pr, extra...).at(b / pr.regions, &vi, &vj);
    const uint32_t src_row = vi * pr.rows_per_video + region, dst_row = vj * pr.rows_per_video + region;
    const uint32_t src_len = row_len[src_row], dst_len = row_len[dst_row];
    const uint64_t *src_ts = ts + row_ts[src_row], *dst_ts = ts + row_ts[dst_row];
    const uint64_t src_seek = row_seek[src_row], dst_seek = row_seek[dst_row];
    const uint64_t min_duration = pr.min_duration[region];
    auto entry_of = [&](const NeedleHipRun &r, DeviceEntry *e) {  // false: the reference skips the run (:212-223)
      const uint32_t i = r.src_end, j = r.dst_end, len = r.len;
      if (len == 0 || len > i || len > j || i >= src_len || j >= dst_len) return false;
      e->src_start = src_ts[i - len] + src_seek;
      e->src_end = src_ts[i] + src_seek;
      e->dst_start = dst_ts[j - len] + dst_seek;
      e->dst_end = dst_ts[j] + dst_seek;
      if (e->src_end < e->src_start || e->dst_end < e->dst_start) return false;
      if (e->src_end - e->src_start < min_duration || e->dst_end - e->dst_start < min_duration) return false;
      e->score = len;
      e->src_hash = r.src_match_hash;
      e->dst_hash = r.dst_match_hash;
      e->pad = 0;
      return true;
    };
    for (uint32_t a = t; a < n; a += 256) {
      const uint32_t idx = (uint32_t)arr[a];
      const NeedleHipRun r = sorted[lo + idx];
      DeviceEntry e;
      const bool ok = entry_of(r, &e);
      const unsigned long long rank = ((unsigned long long)r.len << 32) | ((unsigned long long)((r.src_end - r.len) & 0xFFFFu) << 16) | (r.dst_end & 0xFFFFu);
      arr[a] = (rank << 16) | (ok ? 0x8000ull : 0ull) | idx;
    }
    __syncthreads();
    if (t == 0) {
      uint32_t out = 0;
      for (uint32_t a = 0; a < n; a++) {
        const unsigned long long e = arr[a];
        if (!(e & 0x8000ull)) continue;
        uint32_t pos = out++;
        while (pos > 0) {  // BinaryHeap::push: append, sift up while greater than the parent
          const uint32_t parent = (pos - 1) / 2;
          const unsigned long long p = arr[parent];
          if (!((e >> 16) > (p >> 16))) break;
          arr[pos] = p;
          pos = parent;
        }
        arr[pos] = e;
      }
      heap_size = out;
      valid[b] = out;
    }
    __syncthreads();
    const uint32_t out = heap_size;
    for (uint32_t pos = t; pos < out; pos += 256) {
      const NeedleHipRun r = sorted[lo + (uint32_t)(arr[pos] & 0x1FFFull)];
      DeviceEntry e;
      (void)entry_of(r, &e);
      entries[lo + pos] = e;
    }
    __syncthreads();
  }
}

struct BestKey {
  float score;
  uint32_t index;
  uint32_t have;
};
__device__ __forceinline__ bool better(const BestKey &a, const BestKey &b) {  // a before b in the ascending (score, index) order
  if (!a.have) return false;
  if (!b.have) return true;
  return a.score < b.score || (a.score == b.score && a.index < b.index);
}

__device__ __forceinline__ float as_secs_f32(uint64_t d) {  // Duration::as_secs_f32 (hostutil.cpp duration_as_secs_f32)
  const float secs = (float)(d / 1000000000ull);
  const float frac = (float)(uint32_t)(d % 1000000000ull) / 1000000000.0f;
  return secs + frac;
}

constexpr int kImageRows = 512;   // candidates of a stage of the links' b side (best_match_kernel)
constexpr int kImagePitch = 12;   // words per row of the stage's image: 8 of +-1 bytes + 4 (16-byte reads of sixteen rows: sixteen groups of banks)
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
// Which videos best_match_kernel's workgroups take, where a video's pairs' buckets are and where its result goes.  Built in the
// kernel from EpilogueParams and the kernel's trailing arguments (none for the library job's form: its code is what it was).
struct RowMajorVideos {  // the library job: videos [v0, v1), buckets in the i-major pair order over n videos, results[v]
  uint64_t n;
  uint32_t v0;
  uint64_t hash_duration;
  __device__ explicit RowMajorVideos(const EpilogueParams &pr) : n(pr.n), v0(pr.v0), hash_duration(pr.hash_duration) {}
  __device__ bool live(uint32_t) const { return true; }
  __device__ uint32_t video(uint32_t block) const { return v0 + block; }
  __device__ uint64_t pair(uint32_t q, uint32_t v) const {  // (q, v) for q < v, then (v, q + 1)
    return q < v ? row_start(n, q) + (v - q - 1) : row_start(n, v) + (q - v);
  }
  __device__ uint32_t out(uint32_t, uint32_t v) const { return v; }
  __device__ uint64_t video_hash_duration(uint32_t) const { return hash_duration; }
};
struct IndexVideos {  // an index append: the videos listed (*count of them), buckets in the store's j-major order, results[block]
  const uint32_t *list, *count;
  const uint64_t *hash_durations;  // per video: a candidate of video v is always v's side of its pair (comparator.rs:410-432)
  __device__ IndexVideos(const EpilogueParams &, const uint32_t *l, const uint32_t *c, const uint64_t *hd)
      : list(l), count(c), hash_durations(hd) {}
  __device__ bool live(uint32_t block) const { return block < *count; }
  __device__ uint32_t video(uint32_t block) const { return list[block]; }
  __device__ uint64_t pair(uint32_t q, uint32_t v) const { return q < v ? column_start(v) + q : column_start(q + 1) + v; }
  __device__ uint32_t out(uint32_t block, uint32_t) const { return block; }
  __device__ uint64_t video_hash_duration(uint32_t v) const { return hash_durations[v]; }
};

// One workgroup per wanted video.
template <class Videos, class... Extra>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void best_match_kernel(EpilogueParams pr, const uint32_t *__restrict__ start,
                                                         const uint32_t *__restrict__ valid, const DeviceEntry *__restrict__ entries,
                                                         Candidate *__restrict__ cand_pool, unsigned long long *__restrict__ cand_cursor,
                                                         uint32_t *__restrict__ links_pool, NeedleHipSearchResult *__restrict__ results,
                                                         uint32_t *__restrict__ failed, Extra... extra) {
  __shared__ uint32_t scan[256];
  __shared__ uint32_t carry;
  __shared__ unsigned long long pool_base;
  __shared__ __attribute__((aligned(16))) uint32_t image[kImageRows * kImagePitch];
  __shared__ uint32_t ntab[16];
  __shared__ uint32_t dlinks[2048];
  __shared__ uint32_t distinct;
  __shared__ uint32_t slot_cnt[256], slot_at[256];
  __shared__ uint16_t occupied[1536 + 256];
  __shared__ BestKey best[2][256];
  // a bucket too large for one lane (pair_entries_kernel): the whole job is the host form's, nothing here would be read
  if (__builtin_nontemporal_load(failed) & kEpilogueBucketTooLarge) return;
  const Videos videos(pr, extra...);
  if (!videos.live(blockIdx.x)) return;
  const uint32_t v = videos.video(blockIdx.x), t = threadIdx.x;
  const uint32_t slots = pr.n - 1;  // the video's pairs in lexicographic order: (q, v) for q < v, then (v, q + 1)
  auto bucket_of = [&](uint32_t q) -> uint64_t { return videos.pair(q, v) * pr.regions; };
  // pass 1: candidates per pair slot -> total
  if (t == 0) carry = 0;
  __syncthreads();
  uint32_t mine_total = 0;
  for (uint32_t q = t; q < slots; q += 256) {
    const uint64_t b = bucket_of(q);
    mine_total += valid[b] + (pr.regions == 2 ? valid[b + 1] : 0u);
  }
  scan[t] = mine_total;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)t < d) scan[t] += scan[t + d];
    __syncthreads();
  }
  const uint32_t c = scan[0];
  __syncthreads();
  NeedleHipSearchResult res;
  memset(&res, 0, sizeof(res));
  if (c == 0) {  // no pair of this video has an entry: the reference pushes nothing for it (:608-617)
    if (t == 0) results[videos.out(blockIdx.x, v)] = res;
    return;
  }
  if (t == 0) pool_base = atomicAdd(cand_cursor, (unsigned long long)c);
  __syncthreads();
  Candidate *cand = cand_pool + pool_base;
  uint32_t *links = links_pool + pool_base;
  // pass 2: candidate index of every pair slot (exclusive scan in slot order, 256 slots at a time), then the fill
  for (uint32_t base = 0; base < slots; base += 256) {
    const uint32_t q = base + t;
    uint32_t cnt = 0;
    uint64_t b = 0;
    if (q < slots) {
      b = bucket_of(q);
      cnt = valid[b] + (pr.regions == 2 ? valid[b + 1] : 0u);
    }
    scan[t] = cnt;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const uint32_t add = (int)t >= d ? scan[t - d] : 0u;
      __syncthreads();
      scan[t] += add;
      __syncthreads();
    }
    uint32_t at = carry + scan[t] - cnt;
    // a slot's entries -> candidates: by its own thread while they are few; a slot with many (a pair of silent stretches: hundreds)
    // by the whole workgroup -- one thread copying 400 entries while 255 wait was most of this kernel on the hostile corpus
    auto copy_entries = [&](const uint64_t bb, const bool as_source, uint32_t first, const uint32_t k0, const uint32_t kstep) {
      for (uint32_t r = 0; r < pr.regions; r++) {  // openings first, then endings (:414-431)
        const DeviceEntry *e = entries + start[bb + r];
        const uint32_t k1 = valid[bb + r];
        for (uint32_t k = k0; k < k1; k += kstep) {
          Candidate cd;
          cd.start = as_source ? e[k].src_start : e[k].dst_start;
          cd.end = as_source ? e[k].src_end : e[k].dst_end;
          cd.hash = as_source ? e[k].src_hash : e[k].dst_hash;
          cd.is_opening = r == 0 ? 1u : 0u;
          cand[first + k] = cd;
        }
        first += k1;
      }
    };
    constexpr uint32_t kOwnCopy = 16;
    slot_cnt[t] = cnt;
    slot_at[t] = at;
    if (cnt && cnt <= kOwnCopy) copy_entries(b, q >= v, at, 0u, 1u);
    __syncthreads();
    for (uint32_t qq = 0; qq < 256; qq++) {
      if (slot_cnt[qq] <= kOwnCopy) continue;  // (uniform)
      const uint32_t q2 = base + qq;
      copy_entries(bucket_of(q2), q2 >= v, slot_at[qq], t, 256u);
    }
    __syncthreads();
    if (t == 255) carry += scan[255];
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  // links[k] = #{b : popcount(h_k ^ h_b) < bound}, k itself included (:434-454): all candidates against all -- c x c Hamming
  // distances, 25 million per video at 2000 videos, and as in the scan a matrix product: with a hash as 32 bytes of +-1,
  // dot(a, b) = 32 - 2 d(a, b).  One v_mfma_i32_32x32x32_i8 is 32 candidates b (rows, the A side NEGATED) x 32 candidates k
  // (columns): with the accumulator preset to 32 - 2 bound its sign bit says d < bound.  A lane holds sixteen rows of ITS
  // column: the sixteen sign bits are shifted into a word, two tiles' words counted with one v_bcnt -- 18 vector
  // instructions per 1024 pairs (on the vector ALU, one lane per k: xor, popcount, compare, add = 64).  The b side is
  // staged through LDS as +-1 bytes, kImageRows candidates at a time, built by the workgroup and read by its four waves
  // as A fragments; a wave owns every fourth block of 32 k and keeps their sums in links[] between the stages.
  // (Rows beyond c are zero bytes: dot 0, "d = 16" -- counted as a match when bound > 16 and taken out again below.)
  // Round 6: a video with thousands of candidates has them from stretches of ONE repeated hash (silence, a sustained chord: every
  // diagonal of an S x S block is a run, and the simhash of a constant stretch is that constant) -- 33 000 candidates per video on
  // the hostile corpus at 280 files, a handful of DISTINCT hashes among them.  Candidates of equal hash have equal link counts:
  // links = sum over the distinct hashes within the bound of their multiplicities.  A 2048-slot table in LDS (the image's bytes,
  // unused on this path) takes the hashes by 64-bit compare-and-swap; beyond 1536 distinct values the all-pairs products below run.
  bool deduped = false;
  if (c >= 512) {
    constexpr uint32_t kSlots = 2048, kMaxDistinct = 1536;
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(image);   // 1 << 32 | hash, 0 = empty
    uint32_t *mult = image + 2 * kSlots;
    for (uint32_t i = t; i < kSlots; i += 256) {
      keys[i] = 0ull;
      mult[i] = 0u;
      dlinks[i] = 0u;
    }
    if (t == 0) distinct = 0;
    __syncthreads();
    auto slot_of = [](uint32_t hash) { return (hash * 0x9E3779B1u) >> 21; };
    for (uint32_t k = t; k < c; k += 256) {
      const uint32_t hash = cand[k].hash;
      const unsigned long long want = (1ull << 32) | hash;
      uint32_t sl = slot_of(hash);
      for (uint32_t probe = 0; probe < kSlots; probe++, sl = (sl + 1) & (kSlots - 1)) {
        if (*reinterpret_cast<volatile uint32_t *>(&distinct) > kMaxDistinct) break;  // (overflowing: the direct path will run)
        unsigned long long old = *reinterpret_cast<volatile unsigned long long *>(&keys[sl]);  // (mostly there already: no atomic)
        if (old == 0ull) {
          old = atomicCAS(&keys[sl], 0ull, want);
          if (old == 0ull) atomicAdd(&distinct, 1u);
        }
        if (old == 0ull || old == want) {
          atomicAdd(&mult[sl], 1u);
          break;
        }
      }
    }
    __syncthreads();
    deduped = distinct <= kMaxDistinct;
    if (deduped) {
      if (t == 0) distinct = 0;  // now: the occupied slots, listed
      __syncthreads();
      for (uint32_t a = t; a < kSlots; a += 256)
        if (keys[a] != 0ull) occupied[atomicAdd(&distinct, 1u)] = (uint16_t)a;
      __syncthreads();
      const uint32_t u = distinct;
      for (uint32_t ia = t; ia < u; ia += 256) {
        const uint32_t a = occupied[ia];
        const uint32_t ha = (uint32_t)keys[a];
        uint32_t sum = 0;
        for (uint32_t ib = 0; ib < u; ib++) {
          const uint32_t b2 = occupied[ib];
          if ((uint32_t)__popc(ha ^ (uint32_t)keys[b2]) < pr.bound) sum += mult[b2];
        }
        dlinks[a] = sum;
      }
      __syncthreads();
      for (uint32_t k = t; k < c; k += 256) {
        const uint32_t hash = cand[k].hash;
        const unsigned long long want = (1ull << 32) | hash;
        uint32_t sl = slot_of(hash);
        while (keys[sl] != want) sl = (sl + 1) & (kSlots - 1);                 // present by construction
        links[k] = dlinks[sl];
      }
    }
    __syncthreads();
  }
  if (!deduped) {
    const uint32_t lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    if (t < 16) {
      uint32_t w = 0;
      for (int i = 0; i < 4; i++) w |= (((t >> i) & 1) ? 0x01u : 0xFFu) << (8 * i);
      ntab[t] = w;
    }
    const int preset = 32 - 2 * (int)pr.bound;
    v16i presets;
#pragma unroll
    for (int q = 0; q < 16; q++) presets[q] = preset;
    const uint32_t k_blocks = (c + 31) / 32;
    for (uint32_t b0 = 0; b0 < c; b0 += kImageRows) {
      const uint32_t len = min((uint32_t)kImageRows, c - b0);
      const uint32_t b_blocks = (len + 31) / 32;
      __syncthreads();
      // the stage's image: row i = candidate b0 + i as 32 NEGATED +-1 bytes (a set bit: -1), 8 words at a pitch of 12
      for (uint32_t i = t; i < b_blocks * 32; i += 256) {
        const uint32_t hb = i < len ? ~cand[b0 + i].hash : 0u;
#pragma unroll
        for (int q = 0; q < 8; q++) image[i * kImagePitch + q] = i < len ? ntab[(hb >> (4 * q)) & 0xFu] : 0u;
      }
      __syncthreads();
      const uint32_t pad = b_blocks * 32 - len;   // zero rows of the stage's last block
      for (uint32_t kb = wave; kb < k_blocks; kb += 4) {
        const uint32_t k = kb * 32 + r;
        const uint32_t half = (k < c ? cand[k].hash : 0u) >> (16 * h);
        v4i fb;                                   // B fragment: column r = candidate k, bits 16 h .. 16 h + 15 as +-1 bytes
#pragma unroll
        for (int q = 0; q < 4; q++) fb[q] = (int)ntab[(half >> (4 * q)) & 0xFu];
        uint32_t cnt = 0, word = 0;
        for (uint32_t bb = 0; bb < b_blocks; bb++) {
          const v4i fa = *reinterpret_cast<const v4i *>(image + (bb * 32 + r) * kImagePitch + 4 * h);
          const v16i acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, presets, 0, 0, 0);
#pragma unroll
          for (int q = 0; q < 16; q++) word = __builtin_amdgcn_alignbit(word, (uint32_t)acc[q], 31);
          if (bb & 1) {
            cnt += (uint32_t)__popc(word);
            word = 0;
          }
        }
        cnt += (uint32_t)__popc(word);
        cnt += (uint32_t)__shfl_xor((int)cnt, 32);   // the column's other sixteen rows of every tile
        if (preset < 0) cnt -= pad;               // bound > 16: the zero rows counted
        if (h == 0 && k < c) links[k] = (b0 == 0 ? 0u : links[k]) + cnt;
      }
    }
  }
  __syncthreads();
  // score = -(count * 0.3 + secs * 0.7) in f32, no fused multiply-add (:469); ascending (score, index), first (:473-475)
  BestKey mine[2] = {{0.f, 0u, 0u}, {0.f, 0u, 0u}};
  for (uint32_t k = t; k < c; k += 256) {
    const Candidate cd = cand[k];
    const uint32_t l = links[k];
    if (l == 0) continue;
    const float count = (float)(long long)l;
    const float secs = as_secs_f32(cd.end - cd.start);
    const float a = count * 0.3f;
    const float b = secs * 0.7f;
    const float weighted = a + b;
    const BestKey key = {-weighted, k, 1u};
    const int which = cd.is_opening ? 0 : 1;
    if (better(key, mine[which])) mine[which] = key;
  }
  best[0][t] = mine[0];
  best[1][t] = mine[1];
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)t < d) {
      if (better(best[0][t + d], best[0][t])) best[0][t] = best[0][t + d];
      if (better(best[1][t + d], best[1][t])) best[1][t] = best[1][t + d];
    }
    __syncthreads();
  }
  if (t == 0) {
    res.has_result = true;  // Some(best) even if neither side is found (:514)
    bool bad = false;
    for (int which = 0; which < 2; which++) {
      if (which == 1 && !pr.include_endings) break;  // :486
      const BestKey w = best[which][0];
      if (!w.have) continue;
      const Candidate cd = cand[w.index];
      const uint64_t hash_duration = videos.video_hash_duration(v);
      if (cd.end < pr.time_padding || cd.end - pr.time_padding < hash_duration) {  // Duration underflow panics upstream
        bad = true;
        break;
      }
      const uint64_t s = cd.start + pr.time_padding;                 // :479
      const uint64_t e = cd.end - pr.time_padding - hash_duration;   // :481
      if (which == 0) {
        res.has_opening = true;
        res.opening_start_ns = s;
        res.opening_end_ns = e;
      } else {
        res.has_ending = true;
        res.ending_start_ns = s;
        res.ending_end_ns = e;
      }
    }
    if (bad) atomicAdd(failed, 1u);
    results[videos.out(blockIdx.x, v)] = res;
  }
}

// ---- the incremental index's store (index.cpp) ----------------------------------------------------------------------------
// The append's buckets into the store: start = where the entries were written (the store's entry count before the append plus
// the bucket's start in the append's counting sort), valid = the heap's size.
__global__ __launch_bounds__(256) void index_store_buckets_kernel(uint32_t buckets, const uint32_t *__restrict__ local_start,
                                                                  const uint32_t *__restrict__ local_valid, uint32_t entries_base,
                                                                  uint32_t *__restrict__ store_start, uint32_t *__restrict__ store_valid) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < buckets; b += gridDim.x * blockDim.x) {
    store_start[b] = entries_base + local_start[b];
    store_valid[b] = local_valid[b];
  }
}

// The videos whose candidate list an append changed: an old video i with an entry in a new pair (i, j).  `valid` = the new
// buckets' counts in the store, `first` = the append's first pair id.
__global__ __launch_bounds__(256) void index_changed_kernel(uint32_t buckets, uint32_t regions, uint64_t first,
                                                            const uint32_t *__restrict__ valid, uint32_t *__restrict__ flag) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < buckets; b += gridDim.x * blockDim.x) {
    if (valid[b] == 0) continue;
    uint32_t i, j;
    column_pair_at(first + b / regions, &i, &j);
    flag[i] = 1u;
  }
}
// ... listed, with every new video [n0, n1) (its result is computed even when it has no candidate: then it is "none")
__global__ __launch_bounds__(256) void index_list_kernel(uint32_t n0, uint32_t n1, const uint32_t *__restrict__ flag,
                                                         uint32_t *__restrict__ count, uint32_t *__restrict__ list) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n1; v += gridDim.x * blockDim.x)
    if (v >= n0 || flag[v]) list[atomicAdd(count, 1u)] = v;
}

// ---- an index edit (removal / replacement): the store rebuilt under the new pair ids into the second set of buffers ----
// The kept rows of the hash arena or of the timestamp table into the new one: a workgroup per row, consecutive elements.
template <class T>
__global__ __launch_bounds__(256) void index_copy_rows_kernel(const IndexSegment *__restrict__ rows, uint32_t num_rows,
                                                              const T *__restrict__ from, T *__restrict__ to) {
  for (uint32_t s = blockIdx.x; s < num_rows; s += gridDim.x) {
    const IndexSegment g = rows[s];
    for (uint64_t k = threadIdx.x; k < g.len; k += blockDim.x) to[g.dst + k] = from[g.src + k];
  }
}

// A bucket of the rebuilt store whose pair is kept: its count and where its entries lie in the committed store.  Removal keeps
// the relative order, so the old pair is (old i, old j) with the same roles.  The pairs with a fresh video are left to
// index_edit_fresh_kernel.
__global__ __launch_bounds__(256) void index_edit_buckets_kernel(uint32_t buckets, uint32_t regions, const uint32_t *__restrict__ old_of_new,
                                                                 const uint32_t *__restrict__ old_start, const uint32_t *__restrict__ old_valid,
                                                                 uint32_t *__restrict__ src, uint32_t *__restrict__ count) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < buckets; b += gridDim.x * blockDim.x) {
    uint32_t i, j;
    column_pair_at(b / regions, &i, &j);
    const uint32_t oi = old_of_new[i], oj = old_of_new[j];
    if (oi == kIndexFresh || oj == kIndexFresh) continue;
    const uint64_t ob = (column_start(oj) + oi) * regions + b % regions;
    src[b] = old_start[ob];
    count[b] = old_valid[ob];
  }
}
// ... and a listed pair's bucket: its entries were written behind the committed ones (`base`) by this edit
__global__ __launch_bounds__(256) void index_edit_fresh_kernel(uint32_t listed, uint32_t regions, const uint32_t *__restrict__ pair_ids,
                                                               const uint32_t *__restrict__ lstart, const uint32_t *__restrict__ lvalid,
                                                               uint32_t base, uint32_t *__restrict__ src, uint32_t *__restrict__ count) {
  for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < listed; l += gridDim.x * blockDim.x) {
    const uint64_t b = (uint64_t)pair_ids[l / regions] * regions + l % regions;
    src[b] = base + lstart[l];
    count[b] = lvalid[l];
  }
}

// Every bucket's valid entries to its new start (start[0..buckets], start[buckets] = the total), so that the slots in use are
// the entries held.  A lane per 16-byte word (an entry is three): consecutive lanes move consecutive words; a lane finds its
// bucket by a binary search of the starts, the last one at or below its entry (empty buckets share their start).
__global__ __launch_bounds__(256) void index_gather_kernel(uint32_t buckets, const uint32_t *__restrict__ start,
                                                           const uint32_t *__restrict__ src, const uint4 *__restrict__ from,
                                                           uint4 *__restrict__ to, uint64_t max_entries) {
  const uint64_t words = 3 * min((uint64_t)start[buckets], max_entries);
  for (uint64_t w = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; w < words; w += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t e = (uint32_t)(w / 3);
    uint32_t lo = 0, hi = buckets;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) / 2;
      if (start[mid] <= e) lo = mid;
      else hi = mid;
    }
    to[w] = from[((uint64_t)src[lo] + (e - start[lo])) * 3 + w % 3];
  }
}

// The videos whose candidate list an edit changed: every fresh video ...
__global__ __launch_bounds__(256) void index_fresh_flags_kernel(uint32_t n, const uint32_t *__restrict__ old_of_new, uint32_t *__restrict__ flag) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) flag[v] = old_of_new[v] == kIndexFresh ? 1u : 0u;
}
// ... every kept video with an entry in a pair of a video removed or replaced (the committed store, old ids) ...
__global__ __launch_bounds__(256) void index_gone_partners_kernel(uint32_t n_old, uint32_t regions, const uint32_t *__restrict__ gone,
                                                                  uint32_t num_gone, const uint32_t *__restrict__ valid,
                                                                  const uint32_t *__restrict__ new_of_old, uint32_t *__restrict__ flag) {
  const uint64_t total = (uint64_t)num_gone * n_old;
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t x = gone[t / n_old], q = (uint32_t)(t % n_old);
    if (q == x || new_of_old[q] == kIndexFresh) continue;
    const uint64_t p = q < x ? column_start(x) + q : column_start(q) + x;
    bool any = false;
    for (uint32_t r = 0; r < regions; r++) any = any || valid[p * regions + r] != 0;
    if (any) flag[new_of_old[q]] = 1u;
  }
}
// ... and every video with an entry in a listed pair
__global__ __launch_bounds__(256) void index_fresh_partners_kernel(uint32_t listed, uint32_t regions, const uint32_t *__restrict__ pair_ids,
                                                                   const uint32_t *__restrict__ lvalid, uint32_t *__restrict__ flag) {
  for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < listed; l += gridDim.x * blockDim.x) {
    if (lvalid[l] == 0) continue;
    uint32_t i, j;
    column_pair_at(pair_ids[l / regions], &i, &j);
    flag[i] = 1u;
    flag[j] = 1u;
  }
}

// A device array that keeps its contents when it grows (amortised doubling, a device-to-device copy on `stream`).
template <class T>
struct GrowBuffer {
  DeviceBuffer<T> buf;
  Status reserve(size_t n, size_t keep, hipStream_t stream) {
    if (n <= buf.count) return Status::Ok();
    const size_t want = std::max<size_t>(n, 2 * buf.count);
    T *p = nullptr;
    NEEDLE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), want * sizeof(T)));
    if (keep && buf.ptr) {
      const hipError_t e = hipMemcpyAsync(p, buf.ptr, keep * sizeof(T), hipMemcpyDeviceToDevice, stream);
      const hipError_t w = e == hipSuccess ? hipStreamSynchronize(stream) : e;  // (the old buffer is released below)
      if (w != hipSuccess) {
        (void)hipFree(p);
        return Status::Make(NeedleError_Unknown, std::string("HIP error: ") + hipGetErrorString(w) + " growing an index buffer");
      }
    }
    buf.release();
    buf.ptr = p;
    buf.count = want;
    return Status::Ok();
  }
  T *ptr() const { return buf.ptr; }
};

struct EpilogueWorkspace {
  DeviceBuffer<uint32_t> count, start, fill, sums, valid, links, ctl, row_len, row_ts, large_list;
  bool large_checked = false;
  bool large_ok = false, large_attr_set = false;  // of the resident row tables: every row under 65 536 hashes, timestamps strictly increasing
  DeviceBuffer<uint64_t> row_seek, ts;
  DeviceBuffer<NeedleHipRun> sorted;
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
  if (!w) w = new EpilogueWorkspace();
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
                       uint32_t videos_per_rank, int world, uint8_t *d_send, const DirectPlan &plan, hipStream_t stream) {
  if (world < 1 || world > 64 || n < 2 || regions < 1 || videos_per_rank < 1)
    return Status::Make(NeedleError_InvalidArgument, "directed run exchange: invalid plan");
  for (int q = 0; q < world; q++) NEEDLE_HIP_TRY(hipMemsetAsync(d_send + plan.offset[q], 0, 32, stream));
  const uint32_t grid = (uint32_t)std::min<uint64_t>(2048, ((uint64_t)slab_capacity + 255) / 256);
  hipLaunchKernelGGL(direct_runs_kernel, dim3(std::max(grid, 1u)), dim3(256), 0, stream, d_found, d_runs, slab_capacity, n, regions,
                     videos_per_rank, world, d_send, plan);
  NEEDLE_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

Status gpu_epilogue_enqueue(const EpilogueJob &job, hipStream_t stream, NeedleHipSearchResult *host_results, uint32_t *host_failed) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());  // the per-device workspaces are shared, as everywhere else
  if (job.num_segments < 1 || job.num_segments > kMaxSegments)
    return Status::Make(NeedleError_InvalidArgument, "device epilogue: too many run segments");
  const uint64_t np = (uint64_t)job.n * (job.n - 1) / 2;
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
  const size_t runs = std::max<uint64_t>(job.max_runs, 1);
  if (!(s = ws->count.reserve(buckets)).ok() || !(s = ws->fill.reserve(buckets)).ok() || !(s = ws->start.reserve(buckets + 1)).ok() ||
      !(s = ws->valid.reserve(buckets)).ok() || !(s = ws->sums.reserve((buckets + kScanBlock - 1) / kScanBlock + 1)).ok() ||
      !(s = ws->sorted.reserve(runs)).ok() || !(s = ws->entries.reserve(runs)).ok() || !(s = ws->cand.reserve(2 * runs)).ok() ||
      !(s = ws->links.reserve(2 * runs)).ok() || !(s = ws->ctl.reserve(4)).ok() || !(s = ws->results.reserve(job.n)).ok() ||
      !(s = ws->large_list.reserve(runs / (kEpilogueBucketLimit + 1) + 1)).ok())
    return s;
  if (!ws->large_attr_set) {
    NEEDLE_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pair_entries_large_kernel<RowMajorPairs>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)(kEpilogueLargeLimit * sizeof(unsigned long long))));
    ws->large_attr_set = true;
  }
  RunSegments segs;
  std::memset(&segs, 0, sizeof(segs));
  segs.count = job.num_segments;
  for (int k = 0; k < job.num_segments; k++) {
    segs.found[k] = job.segment_count[k];
    segs.runs[k] = job.segment_runs[k];
    segs.capacity[k] = job.segment_capacities[k] ? job.segment_capacities[k] : job.segment_capacity;
  }
  EpilogueParams pr;
  std::memset(&pr, 0, sizeof(pr));
  pr.n = job.n;
  pr.regions = job.regions;
  pr.rows_per_video = job.rows_per_video;
  pr.buckets = (uint32_t)buckets;
  pr.v0 = job.v0;
  pr.v1 = job.v1;
  pr.bound = job.threshold + job.threshold / 2;
  pr.include_endings = job.include_endings ? 1u : 0u;
  pr.min_duration[0] = job.min_opening_duration;
  pr.min_duration[1] = job.min_ending_duration;
  pr.time_padding = job.time_padding;
  pr.hash_duration = job.hash_duration;
  pr.large_ok = ws->large_ok && getenv("NEEDLE_HIP_EPILOGUE_NO_LARGE") == nullptr ? 1u : 0u;  // (tests: the host fallback itself)
  NEEDLE_HIP_TRY(hipMemsetAsync(ws->count.ptr, 0, buckets * sizeof(uint32_t), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(ws->fill.ptr, 0, buckets * sizeof(uint32_t), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(ws->ctl.ptr, 0, 4 * sizeof(uint32_t), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(ws->results.ptr, 0, (size_t)job.n * sizeof(NeedleHipSearchResult), stream));
  const uint32_t run_grid = (uint32_t)std::min<uint64_t>(4096, (runs + 255) / 256);
  const uint32_t scan_blocks = (uint32_t)((buckets + kScanBlock - 1) / kScanBlock);
  {
    KernelTimer timer("epilogue_buckets", stream);
    hipLaunchKernelGGL(bucket_count_kernel, dim3(run_grid), dim3(256), 0, stream, segs, pr.buckets, ws->count.ptr);
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(scan_blocks), dim3(256), 0, stream, ws->count.ptr, pr.buckets, ws->sums.ptr);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, ws->sums.ptr, scan_blocks);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(scan_blocks), dim3(256), 0, stream, ws->count.ptr, pr.buckets, ws->sums.ptr, ws->start.ptr);
    hipLaunchKernelGGL(bucket_scatter_kernel, dim3(run_grid), dim3(256), 0, stream, segs, pr.buckets, ws->start.ptr, ws->fill.ptr,
                       ws->sorted.ptr);
  }
  {
    KernelTimer timer("epilogue_entries", stream);
    hipLaunchKernelGGL(pair_entries_kernel<RowMajorPairs>, dim3((pr.buckets + 63) / 64), dim3(64), 0, stream, pr, ws->start.ptr, ws->sorted.ptr,
                       ws->row_len.ptr, ws->row_ts.ptr, ws->row_seek.ptr, ws->ts.ptr, ws->entries.ptr, ws->valid.ptr, ws->ctl.ptr + 2,
                       ws->ctl.ptr + 3, ws->large_list.ptr);
    // the buckets one lane should not order (a stride loop over a list that is empty on ordinary audio: ~2 us then)
    hipLaunchKernelGGL(pair_entries_large_kernel<RowMajorPairs>, dim3(512), dim3(256), kEpilogueLargeLimit * sizeof(unsigned long long), stream, pr,
                       ws->start.ptr, ws->sorted.ptr, ws->row_len.ptr, ws->row_ts.ptr, ws->row_seek.ptr, ws->ts.ptr, ws->entries.ptr,
                       ws->valid.ptr, ws->ctl.ptr + 3, ws->large_list.ptr);
  }
  if (pr.v1 > pr.v0) {
    KernelTimer timer("epilogue_best_match", stream);
    hipLaunchKernelGGL(best_match_kernel<RowMajorVideos>, dim3(pr.v1 - pr.v0), dim3(256), 0, stream, pr, ws->start.ptr, ws->valid.ptr, ws->entries.ptr,
                       ws->cand.ptr, reinterpret_cast<unsigned long long *>(ws->ctl.ptr), ws->links.ptr, ws->results.ptr, ws->ctl.ptr + 2);
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  NEEDLE_HIP_TRY(hipMemcpyAsync(host_results, ws->results.ptr, (size_t)job.n * sizeof(NeedleHipSearchResult), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(host_failed, ws->ctl.ptr + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  return Status::Ok();
}


// ---- the incremental index's store -------------------------------------------------------------------------------------------
static_assert(sizeof(IndexEntry) == sizeof(DeviceEntry) && offsetof(IndexEntry, score) == offsetof(DeviceEntry, score) &&
                  offsetof(IndexEntry, dst_hash) == offsetof(DeviceEntry, dst_hash),
              "IndexEntry mirrors DeviceEntry");

struct IndexStore {
  // committed: what the index holds (an append that fails leaves these, and what lies below them, as they were)
  uint32_t n = 0;
  uint64_t buckets = 0, entries = 0, rows = 0, ts = 0, hashes = 0;
  // resident: the per-pair entries and, per bucket b = p(i, j) * regions + r, where they start and how many
  GrowBuffer<DeviceEntry> entry;
  GrowBuffer<uint32_t> start, valid, row_len, row_ts, hash;
  GrowBuffer<uint64_t> row_seek, ts_table, hash_duration;
  // the second set an edit gathers the rebuilt store into (index_store_switch swaps the two)
  GrowBuffer<DeviceEntry> entry2;
  GrowBuffer<uint32_t> start2, valid2, row_len2, row_ts2, hash2;
  GrowBuffer<uint64_t> row_seek2, ts_table2, hash_duration2;
  DeviceBuffer<uint32_t> src, old_of_new, new_of_old, gone, pair_ids;  // an edit's maps
  DeviceBuffer<IndexSegment> segments;
  // an append's scratch
  DeviceBuffer<uint32_t> count, fill, lstart, sums, lvalid, ctl, large_list, flag, list, links, run_count;
  DeviceBuffer<NeedleHipRun> runs, sorted;
  DeviceBuffer<Candidate> cand;
  DeviceBuffer<NeedleHipSearchResult> results;
  void *pinned = nullptr;  // [found, failed, listed, held] + list[n1] + results[n1]
  size_t pinned_bytes = 0;
  uint32_t capacity = 1u << 16;  // of the run list; grows to what an append found
  bool large_attr_set = false, listed_attr_set = false;
  bool used = false;  // an append has enqueued work (a store made without a device never has)
  int device = 0;
  ~IndexStore() {
    if (pinned) (void)hipHostFree(pinned);
  }
};

IndexStore *index_store_new() {
  IndexStore *st = new IndexStore();
  (void)hipGetDevice(&st->device);
  return st;
}
void index_store_free(IndexStore *st) {
  if (!st) return;
  if (!st->used) {
    delete st;
    return;
  }
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  int dev = 0;
  (void)hipGetDevice(&dev);
  const int own = st->device;
  if (dev != own) (void)hipSetDevice(own);
  (void)hipStreamSynchronize(library_stream());  // (no launch of this append may still read the buffers)
  delete st;
  if (dev != own) (void)hipSetDevice(dev);
}

namespace {

template <class Op>  // IndexAppend or IndexEdit; n = the videos after it
EpilogueParams index_params(const Op &a, uint32_t n, uint64_t buckets) {
  EpilogueParams pr;
  std::memset(&pr, 0, sizeof(pr));
  pr.n = n;
  pr.regions = pr.rows_per_video = a.regions;
  pr.buckets = (uint32_t)buckets;
  pr.v0 = 0;
  pr.v1 = n;
  pr.bound = a.threshold + a.threshold / 2;
  pr.include_endings = a.include_endings ? 1u : 0u;
  pr.min_duration[0] = a.min_opening_duration;
  pr.min_duration[1] = a.min_ending_duration;
  pr.time_padding = a.time_padding;
  pr.large_ok = a.large_ok && getenv("NEEDLE_HIP_EPILOGUE_NO_LARGE") == nullptr ? 1u : 0u;
  return pr;
}

// the runs found, the failure word, the listed videos' results (and `held`, an edit's entry count) into pinned memory; the wait
Status index_copy_out(IndexStore *st, uint32_t n, const uint32_t *held, hipStream_t stream, IndexAppendOut *out) {
  uint32_t *head = static_cast<uint32_t *>(st->pinned);
  uint32_t *list = head + 4;
  NeedleHipSearchResult *results = reinterpret_cast<NeedleHipSearchResult *>(list + ((n + 1) & ~1u));
  NEEDLE_HIP_TRY(hipMemcpyAsync(head, st->run_count.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(head + 1, st->ctl.ptr + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(head + 2, st->ctl.ptr + 4, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  if (held) NEEDLE_HIP_TRY(hipMemcpyAsync(head + 3, held, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(list, st->list.ptr, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(results, st->results.ptr, (size_t)n * sizeof(NeedleHipSearchResult), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  out->found = head[0];
  out->failed = head[1];
  out->held = held ? head[3] : 0;
  const uint32_t listed = std::min(head[2], n);
  out->videos.assign(list, list + listed);
  out->results.assign(results, results + listed);
  return Status::Ok();
}

// mark the changed videos, list them, best_match over the list; then the copies into pinned memory and a wait for them
Status index_best_and_copy(IndexStore *st, const IndexAppend &a, uint64_t new_buckets, hipStream_t stream, IndexAppendOut *out) {
  const EpilogueParams pr = index_params(a, a.n1, new_buckets);
  const uint64_t first = (uint64_t)a.n0 * (a.n0 - (a.n0 ? 1 : 0)) / 2;
  NEEDLE_HIP_TRY(hipMemsetAsync(st->flag.ptr, 0, std::max<size_t>(a.n1, 1) * sizeof(uint32_t), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(st->ctl.ptr, 0, 2 * sizeof(uint32_t), stream));  // the candidate cursor
  NEEDLE_HIP_TRY(hipMemsetAsync(st->ctl.ptr + 4, 0, sizeof(uint32_t), stream));  // videos listed
  {
    KernelTimer timer("index_best_match", stream);
    if (new_buckets) {
      const uint32_t grid = (uint32_t)std::min<uint64_t>(4096, (new_buckets + 255) / 256);
      hipLaunchKernelGGL(index_changed_kernel, dim3(grid), dim3(256), 0, stream, (uint32_t)new_buckets, a.regions, first,
                         st->valid.ptr() + st->buckets, st->flag.ptr);
    }
    hipLaunchKernelGGL(index_list_kernel, dim3((a.n1 + 255) / 256), dim3(256), 0, stream, a.n0, a.n1, st->flag.ptr, st->ctl.ptr + 4,
                       st->list.ptr);
    // one workgroup per video at most; those beyond the list's length return at once
    hipLaunchKernelGGL((best_match_kernel<IndexVideos, const uint32_t *, const uint32_t *, const uint64_t *>), dim3(a.n1), dim3(256), 0, stream, pr, st->start.ptr(), st->valid.ptr(),
                       st->entry.ptr(), st->cand.ptr, reinterpret_cast<unsigned long long *>(st->ctl.ptr), st->links.ptr,
                       st->results.ptr, st->ctl.ptr + 2, (const uint32_t *)st->list.ptr, (const uint32_t *)(st->ctl.ptr + 4),
                       (const uint64_t *)st->hash_duration.ptr());
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  return index_copy_out(st, a.n1, nullptr, stream, out);
}

}  // namespace

Status gpu_index_append(IndexStore *st, const IndexAppend &a, IndexAppendOut *out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = ensure_device();
  if (!s.ok()) return s;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != st->device) return Status::Make(NeedleError_InvalidArgument, "index: the current device is not the one the index was created on");
  st->used = true;
  if (a.n0 != st->n || a.n1 <= a.n0 || a.regions < 1 || a.regions > 2)
    return Status::Make(NeedleError_InvalidArgument, "index append: inconsistent sizes");
  hipStream_t stream = library_stream();
  const uint64_t first = (uint64_t)a.n0 * (a.n0 - (a.n0 ? 1 : 0)) / 2;
  const uint64_t new_buckets = ((uint64_t)a.n1 * (a.n1 - 1) / 2 - first) * a.regions;
  const uint64_t rows1 = st->rows + a.num_rows, ts1 = st->ts + a.num_ts, hashes1 = st->hashes + a.num_hashes;
  if (st->buckets + new_buckets >= 0xFFFFFFF0ull || hashes1 > UINT32_MAX)
    return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 hashes or sequence pairs");
  // the resident tables: the new videos' rows, timestamps, hash durations and hashes go in behind the committed ones
  if (!(s = st->hash.reserve(std::max<uint64_t>(hashes1, 1), st->hashes, stream)).ok() ||
      !(s = st->row_len.reserve(rows1, st->rows, stream)).ok() || !(s = st->row_ts.reserve(rows1, st->rows, stream)).ok() ||
      !(s = st->row_seek.reserve(rows1, st->rows, stream)).ok() || !(s = st->ts_table.reserve(std::max<uint64_t>(ts1, 1), st->ts, stream)).ok() ||
      !(s = st->hash_duration.reserve(a.n1, st->n, stream)).ok() ||
      !(s = st->start.reserve(std::max<uint64_t>(st->buckets + new_buckets, 1), st->buckets, stream)).ok() ||
      !(s = st->valid.reserve(std::max<uint64_t>(st->buckets + new_buckets, 1), st->buckets, stream)).ok())
    return s;
  if (a.num_hashes)
    NEEDLE_HIP_TRY(hipMemcpyAsync(st->hash.ptr() + st->hashes, a.hashes, a.num_hashes * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(st->row_len.ptr() + st->rows, a.row_len, a.num_rows * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(st->row_ts.ptr() + st->rows, a.row_ts, a.num_rows * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(st->row_seek.ptr() + st->rows, 0, a.num_rows * sizeof(uint64_t), stream));
  if (a.num_ts) NEEDLE_HIP_TRY(hipMemcpyAsync(st->ts_table.ptr() + st->ts, a.ts, a.num_ts * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(st->hash_duration.ptr() + st->n, a.hash_duration, (size_t)(a.n1 - a.n0) * sizeof(uint64_t),
                                hipMemcpyHostToDevice, stream));
  const size_t pinned_want = 16 + ((size_t)a.n1 + 2) * sizeof(uint32_t) + (size_t)a.n1 * sizeof(NeedleHipSearchResult);
  if (pinned_want > st->pinned_bytes) {
    if (st->pinned) (void)hipHostFree(st->pinned);
    st->pinned = nullptr;
    st->pinned_bytes = 0;
    NEEDLE_HIP_TRY(hipHostMalloc(&st->pinned, 2 * pinned_want, hipHostMallocDefault));
    st->pinned_bytes = 2 * pinned_want;
  }
  st->capacity = (uint32_t)std::min<uint64_t>(0x7fffffffu, std::max<uint64_t>(st->capacity, 3 * (uint64_t)a.num_problems));
  for (int attempt = 0; attempt < 2; attempt++) {
    const uint32_t capacity = st->capacity;
    const uint64_t entries1 = st->entries + capacity;
    if (entries1 >= 0xFFFFFFF0ull) return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 heap entries");
    const uint64_t cand = 2 * entries1;  // every entry is a candidate of its two videos
    if (!(s = st->entry.reserve(entries1, st->entries, stream)).ok() || !(s = st->runs.reserve(capacity)).ok() ||
        !(s = st->sorted.reserve(capacity)).ok() || !(s = st->run_count.reserve(1)).ok() ||
        !(s = st->count.reserve(std::max<uint64_t>(new_buckets, 1))).ok() || !(s = st->fill.reserve(std::max<uint64_t>(new_buckets, 1))).ok() ||
        !(s = st->lstart.reserve(new_buckets + 1)).ok() || !(s = st->lvalid.reserve(std::max<uint64_t>(new_buckets, 1))).ok() ||
        !(s = st->sums.reserve((new_buckets + kScanBlock - 1) / kScanBlock + 1)).ok() || !(s = st->ctl.reserve(8)).ok() ||
        !(s = st->large_list.reserve(capacity / (kEpilogueBucketLimit + 1) + 1)).ok() || !(s = st->flag.reserve(a.n1)).ok() ||
        !(s = st->list.reserve(a.n1)).ok() || !(s = st->results.reserve(a.n1)).ok() || !(s = st->cand.reserve(cand)).ok() ||
        !(s = st->links.reserve(cand)).ok())
      return s;
    if (!st->large_attr_set) {
      NEEDLE_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pair_entries_large_kernel<ColumnMajorPairs, uint64_t>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kEpilogueLargeLimit * sizeof(unsigned long long))));
      st->large_attr_set = true;
    }
    // the scan of the new pairs only (every form eligible), behind the uploads on the same stream
    if (!(s = gpu_hamming_runs_device(st->hash.ptr(), a.seqs, a.num_seqs, a.problems, a.num_problems, a.threshold, st->runs.ptr,
                                      capacity, st->run_count.ptr, false, false)).ok())
      return s;
    NEEDLE_HIP_TRY(hipMemsetAsync(st->ctl.ptr, 0, 8 * sizeof(uint32_t), stream));
    if (new_buckets) {
      RunSegments segs;
      std::memset(&segs, 0, sizeof(segs));
      segs.count = 1;
      segs.found[0] = st->run_count.ptr;
      segs.runs[0] = st->runs.ptr;
      segs.capacity[0] = capacity;
      const EpilogueParams pr = index_params(a, a.n1, new_buckets);
      const uint32_t run_grid = (uint32_t)std::min<uint64_t>(4096, ((uint64_t)capacity + 255) / 256);
      const uint32_t scan_blocks = (uint32_t)((new_buckets + kScanBlock - 1) / kScanBlock);
      NEEDLE_HIP_TRY(hipMemsetAsync(st->count.ptr, 0, new_buckets * sizeof(uint32_t), stream));
      NEEDLE_HIP_TRY(hipMemsetAsync(st->fill.ptr, 0, new_buckets * sizeof(uint32_t), stream));
      {
        KernelTimer timer("index_buckets", stream);
        hipLaunchKernelGGL(bucket_count_kernel, dim3(run_grid), dim3(256), 0, stream, segs, pr.buckets, st->count.ptr);
        hipLaunchKernelGGL(scan_block_sums_kernel, dim3(scan_blocks), dim3(256), 0, stream, st->count.ptr, pr.buckets, st->sums.ptr);
        hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, st->sums.ptr, scan_blocks);
        hipLaunchKernelGGL(scan_apply_kernel, dim3(scan_blocks), dim3(256), 0, stream, st->count.ptr, pr.buckets, st->sums.ptr, st->lstart.ptr);
        hipLaunchKernelGGL(bucket_scatter_kernel, dim3(run_grid), dim3(256), 0, stream, segs, pr.buckets, st->lstart.ptr, st->fill.ptr,
                           st->sorted.ptr);
      }
      {
        KernelTimer timer("index_entries", stream);
        DeviceEntry *entries = st->entry.ptr() + st->entries;  // the new pairs' entries go straight in behind the committed ones
        hipLaunchKernelGGL((pair_entries_kernel<ColumnMajorPairs, uint64_t>), dim3((pr.buckets + 63) / 64), dim3(64), 0, stream, pr,
                           st->lstart.ptr, st->sorted.ptr, st->row_len.ptr(), st->row_ts.ptr(), st->row_seek.ptr(), st->ts_table.ptr(), entries,
                           st->lvalid.ptr, st->ctl.ptr + 2, st->ctl.ptr + 3, st->large_list.ptr, first);
        hipLaunchKernelGGL((pair_entries_large_kernel<ColumnMajorPairs, uint64_t>), dim3(512), dim3(256),
                           kEpilogueLargeLimit * sizeof(unsigned long long), stream, pr, st->lstart.ptr, st->sorted.ptr, st->row_len.ptr(),
                           st->row_ts.ptr(), st->row_seek.ptr(), st->ts_table.ptr(), entries, st->lvalid.ptr, st->ctl.ptr + 3,
                           st->large_list.ptr, first);
        hipLaunchKernelGGL(index_store_buckets_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (new_buckets + 255) / 256)), dim3(256), 0,
                           stream, (uint32_t)new_buckets, st->lstart.ptr, st->lvalid.ptr, (uint32_t)st->entries,
                           st->start.ptr() + st->buckets, st->valid.ptr() + st->buckets);
      }
      NEEDLE_HIP_TRY(hipGetLastError());
    }
    if (!(s = index_best_and_copy(st, a, new_buckets, stream, out)).ok()) return s;
    if (out->found <= capacity) {
      out->runs.clear();
      if ((out->failed & kEpilogueBucketTooLarge) && out->found) {  // the host computes this append's entries (index.cpp)
        out->runs.resize(out->found);
        NEEDLE_HIP_TRY(hipMemcpy(out->runs.data(), st->runs.ptr, (size_t)out->found * sizeof(NeedleHipRun), hipMemcpyDeviceToHost));
      }
      return Status::Ok();
    }
    st->capacity = out->found;  // the scan is deterministic: a second pass with the exact size fits
  }
  return Status::Make(NeedleError_Unknown, "index append: run list did not fit after resize");
}

Status gpu_index_append_host_entries(IndexStore *st, const IndexAppend &a, const std::vector<uint32_t> &start,
                                     const std::vector<uint32_t> &valid, const std::vector<IndexEntry> &entries, IndexAppendOut *out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  hipStream_t stream = library_stream();
  const uint64_t first = (uint64_t)a.n0 * (a.n0 - (a.n0 ? 1 : 0)) / 2;
  const uint64_t new_buckets = ((uint64_t)a.n1 * (a.n1 - 1) / 2 - first) * a.regions;
  if (start.size() != new_buckets || valid.size() != new_buckets || st->entries + entries.size() > st->entry.buf.count)
    return Status::Make(NeedleError_InvalidArgument, "index append: host entries do not fit the append");
  std::vector<uint32_t> shifted(start);
  for (uint32_t &x : shifted) x += (uint32_t)st->entries;
  if (!entries.empty())
    NEEDLE_HIP_TRY(hipMemcpyAsync(st->entry.ptr() + st->entries, entries.data(), entries.size() * sizeof(IndexEntry), hipMemcpyHostToDevice, stream));
  if (new_buckets) {
    NEEDLE_HIP_TRY(hipMemcpyAsync(st->start.ptr() + st->buckets, shifted.data(), new_buckets * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    NEEDLE_HIP_TRY(hipMemcpyAsync(st->valid.ptr() + st->buckets, valid.data(), new_buckets * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  }
  NEEDLE_HIP_TRY(hipMemsetAsync(st->ctl.ptr + 2, 0, sizeof(uint32_t), stream));  // the failure word
  const uint32_t found = out->found;
  Status s = index_best_and_copy(st, a, new_buckets, stream, out);
  out->found = found;
  return s;
}

void index_store_commit(IndexStore *st, const IndexAppend &a, uint32_t found) {
  const uint64_t first = (uint64_t)a.n0 * (a.n0 - (a.n0 ? 1 : 0)) / 2;
  st->buckets += ((uint64_t)a.n1 * (a.n1 - 1) / 2 - first) * a.regions;
  st->entries += found;
  st->rows += a.num_rows;
  st->ts += a.num_ts;
  st->hashes += a.num_hashes;
  st->n = a.n1;
}


// ---- an edit: removal / replacement --------------------------------------------------------------------------------------
namespace {

uint64_t edit_buckets(const IndexEdit &e) { return (uint64_t)e.n_new * (e.n_new ? e.n_new - 1 : 0) / 2 * e.regions; }

// The first half of an edit: the maps and the new rows' tables uploaded, the kept rows gathered into the second arena and
// timestamp table, the fresh rows behind them; the scan of the listed pairs and their entries behind the committed ones.
Status index_edit_tables(IndexStore *st, const IndexEdit &e, uint32_t capacity, hipStream_t stream) {
  const uint32_t R = e.regions;
  const uint64_t rows = (uint64_t)e.n_new * R, listed = (uint64_t)e.num_pairs * R;
  NEEDLE_HIP_TRY(hipMemcpyAsync(st->old_of_new.ptr, e.old_of_new, e.n_new * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(st->new_of_old.ptr, e.new_of_old, e.n_old * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  if (e.num_gone) NEEDLE_HIP_TRY(hipMemcpyAsync(st->gone.ptr, e.gone, e.num_gone * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  if (e.num_pairs) NEEDLE_HIP_TRY(hipMemcpyAsync(st->pair_ids.ptr, e.pair_ids, e.num_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  if (e.num_hash_rows)
    NEEDLE_HIP_TRY(hipMemcpyAsync(st->segments.ptr, e.hash_rows, e.num_hash_rows * sizeof(IndexSegment), hipMemcpyHostToDevice, stream));
  if (e.num_ts_rows)
    NEEDLE_HIP_TRY(hipMemcpyAsync(st->segments.ptr + e.num_hash_rows, e.ts_rows, e.num_ts_rows * sizeof(IndexSegment),
                                  hipMemcpyHostToDevice, stream));
  if (e.num_hashes)
    NEEDLE_HIP_TRY(hipMemcpyAsync(st->hash2.ptr() + (e.total_hashes - e.num_hashes), e.hashes, e.num_hashes * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, stream));
  if (e.num_ts)
    NEEDLE_HIP_TRY(hipMemcpyAsync(st->ts_table2.ptr() + (e.total_ts - e.num_ts), e.ts, e.num_ts * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(st->row_len2.ptr(), e.row_len, rows * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(st->row_ts2.ptr(), e.row_ts, rows * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(st->row_seek2.ptr(), 0, rows * sizeof(uint64_t), stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(st->hash_duration2.ptr(), e.hash_duration, e.n_new * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
  {
    KernelTimer timer("index_copy_rows", stream);
    if (e.num_hash_rows)
      hipLaunchKernelGGL(index_copy_rows_kernel<uint32_t>, dim3((uint32_t)std::min<size_t>(e.num_hash_rows, 4096)), dim3(256), 0, stream,
                         (const IndexSegment *)st->segments.ptr, (uint32_t)e.num_hash_rows, (const uint32_t *)st->hash.ptr(), st->hash2.ptr());
    if (e.num_ts_rows)
      hipLaunchKernelGGL(index_copy_rows_kernel<uint64_t>, dim3((uint32_t)std::min<size_t>(e.num_ts_rows, 4096)), dim3(256), 0, stream,
                         (const IndexSegment *)(st->segments.ptr + e.num_hash_rows), (uint32_t)e.num_ts_rows,
                         (const uint64_t *)st->ts_table.ptr(), st->ts_table2.ptr());
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  NEEDLE_HIP_TRY(hipMemsetAsync(st->ctl.ptr, 0, 8 * sizeof(uint32_t), stream));
  if (!e.num_problems) {
    NEEDLE_HIP_TRY(hipMemsetAsync(st->run_count.ptr, 0, sizeof(uint32_t), stream));
  } else {
    Status s = gpu_hamming_runs_device(st->hash2.ptr(), e.seqs, rows, e.problems, e.num_problems, e.threshold, st->runs.ptr, capacity,
                                       st->run_count.ptr, false, false);
    if (!s.ok()) return s;
  }
  if (!listed) return Status::Ok();
  RunSegments segs;
  std::memset(&segs, 0, sizeof(segs));
  segs.count = 1;
  segs.found[0] = st->run_count.ptr;
  segs.runs[0] = st->runs.ptr;
  segs.capacity[0] = capacity;
  const EpilogueParams pr = index_params(e, e.n_new, listed);
  const uint32_t run_grid = (uint32_t)std::min<uint64_t>(4096, ((uint64_t)capacity + 255) / 256);
  const uint32_t scan_blocks = (uint32_t)((listed + kScanBlock - 1) / kScanBlock);
  NEEDLE_HIP_TRY(hipMemsetAsync(st->count.ptr, 0, listed * sizeof(uint32_t), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(st->fill.ptr, 0, listed * sizeof(uint32_t), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(st->lvalid.ptr, 0, listed * sizeof(uint32_t), stream));  // (a bucket the device does not order: 0)
  {
    KernelTimer timer("index_buckets", stream);
    hipLaunchKernelGGL(bucket_count_kernel, dim3(run_grid), dim3(256), 0, stream, segs, pr.buckets, st->count.ptr);
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(scan_blocks), dim3(256), 0, stream, st->count.ptr, pr.buckets, st->sums.ptr);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, st->sums.ptr, scan_blocks);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(scan_blocks), dim3(256), 0, stream, st->count.ptr, pr.buckets, st->sums.ptr, st->lstart.ptr);
    hipLaunchKernelGGL(bucket_scatter_kernel, dim3(run_grid), dim3(256), 0, stream, segs, pr.buckets, st->lstart.ptr, st->fill.ptr, st->sorted.ptr);
  }
  {
    KernelTimer timer("index_entries", stream);
    DeviceEntry *entries = st->entry.ptr() + st->entries;  // behind the committed entries (not part of the store until gathered)
    const uint32_t *pair_ids = st->pair_ids.ptr;
    hipLaunchKernelGGL((pair_entries_kernel<ListedPairs, const uint32_t *>), dim3((pr.buckets + 63) / 64), dim3(64), 0, stream, pr,
                       st->lstart.ptr, st->sorted.ptr, st->row_len2.ptr(), st->row_ts2.ptr(), st->row_seek2.ptr(), st->ts_table2.ptr(),
                       entries, st->lvalid.ptr, st->ctl.ptr + 2, st->ctl.ptr + 3, st->large_list.ptr, pair_ids);
    hipLaunchKernelGGL((pair_entries_large_kernel<ListedPairs, const uint32_t *>), dim3(512), dim3(256),
                       kEpilogueLargeLimit * sizeof(unsigned long long), stream, pr, st->lstart.ptr, st->sorted.ptr, st->row_len2.ptr(),
                       st->row_ts2.ptr(), st->row_seek2.ptr(), st->ts_table2.ptr(), entries, st->lvalid.ptr, st->ctl.ptr + 3,
                       st->large_list.ptr, pair_ids);
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

// The second half: every bucket's count and source (kept pairs from the committed store, listed ones from this edit's
// entries), their starts, the gather into the second entry buffer, the videos to recompute and their best match over the
// rebuilt store; the copies and the wait.
Status index_edit_rebuild(IndexStore *st, const IndexEdit &e, hipStream_t stream, IndexAppendOut *out) {
  const uint32_t R = e.regions, n = e.n_new;
  const uint64_t buckets = edit_buckets(e), listed = (uint64_t)e.num_pairs * R;
  {
    KernelTimer timer("index_rebuild", stream);
    if (buckets) {
      hipLaunchKernelGGL(index_edit_buckets_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (buckets + 255) / 256)), dim3(256), 0, stream,
                         (uint32_t)buckets, R, (const uint32_t *)st->old_of_new.ptr, (const uint32_t *)st->start.ptr(),
                         (const uint32_t *)st->valid.ptr(), st->src.ptr, st->valid2.ptr());
      if (listed)
        hipLaunchKernelGGL(index_edit_fresh_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (listed + 255) / 256)), dim3(256), 0, stream,
                           (uint32_t)listed, R, (const uint32_t *)st->pair_ids.ptr, (const uint32_t *)st->lstart.ptr,
                           (const uint32_t *)st->lvalid.ptr, (uint32_t)st->entries, st->src.ptr, st->valid2.ptr());
      const uint32_t scan_blocks = (uint32_t)((buckets + kScanBlock - 1) / kScanBlock);
      hipLaunchKernelGGL(scan_block_sums_kernel, dim3(scan_blocks), dim3(256), 0, stream, st->valid2.ptr(), (uint32_t)buckets, st->sums.ptr);
      hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, st->sums.ptr, scan_blocks);
      hipLaunchKernelGGL(scan_apply_kernel, dim3(scan_blocks), dim3(256), 0, stream, st->valid2.ptr(), (uint32_t)buckets, st->sums.ptr,
                         st->start2.ptr());
    } else {
      NEEDLE_HIP_TRY(hipMemsetAsync(st->start2.ptr(), 0, sizeof(uint32_t), stream));
    }
  }
  if (buckets) {
    KernelTimer timer("index_gather", stream);
    const uint64_t max_entries = st->entry2.buf.count;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(8192, (3 * max_entries + 255) / 256);
    hipLaunchKernelGGL(index_gather_kernel, dim3(std::max(grid, 1u)), dim3(256), 0, stream, (uint32_t)buckets, (const uint32_t *)st->start2.ptr(),
                       (const uint32_t *)st->src.ptr, reinterpret_cast<const uint4 *>(st->entry.ptr()),
                       reinterpret_cast<uint4 *>(st->entry2.ptr()), max_entries);
  }
  const EpilogueParams pr = index_params(e, n, buckets);
  NEEDLE_HIP_TRY(hipMemsetAsync(st->ctl.ptr, 0, 2 * sizeof(uint32_t), stream));  // the candidate cursor
  NEEDLE_HIP_TRY(hipMemsetAsync(st->ctl.ptr + 4, 0, sizeof(uint32_t), stream));  // videos listed
  {
    KernelTimer timer("index_best_match", stream);
    hipLaunchKernelGGL(index_fresh_flags_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, (const uint32_t *)st->old_of_new.ptr, st->flag.ptr);
    if (e.num_gone && e.n_old > 1) {
      const uint64_t work = (uint64_t)e.num_gone * e.n_old;
      hipLaunchKernelGGL(index_gone_partners_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (work + 255) / 256)), dim3(256), 0, stream, e.n_old,
                         R, (const uint32_t *)st->gone.ptr, (uint32_t)e.num_gone, (const uint32_t *)st->valid.ptr(),
                         (const uint32_t *)st->new_of_old.ptr, st->flag.ptr);
    }
    if (listed)
      hipLaunchKernelGGL(index_fresh_partners_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (listed + 255) / 256)), dim3(256), 0, stream,
                         (uint32_t)listed, R, (const uint32_t *)st->pair_ids.ptr, (const uint32_t *)st->lvalid.ptr, st->flag.ptr);
    hipLaunchKernelGGL(index_list_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, n, (const uint32_t *)st->flag.ptr, st->ctl.ptr + 4,
                       st->list.ptr);
    hipLaunchKernelGGL((best_match_kernel<IndexVideos, const uint32_t *, const uint32_t *, const uint64_t *>), dim3(n), dim3(256), 0, stream,
                       pr, st->start2.ptr(), st->valid2.ptr(), st->entry2.ptr(), st->cand.ptr,
                       reinterpret_cast<unsigned long long *>(st->ctl.ptr), st->links.ptr, st->results.ptr, st->ctl.ptr + 2,
                       (const uint32_t *)st->list.ptr, (const uint32_t *)(st->ctl.ptr + 4), (const uint64_t *)st->hash_duration2.ptr());
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  return index_copy_out(st, n, st->start2.ptr() + buckets, stream, out);
}

template <class T>
void swap_buffers(GrowBuffer<T> &a, GrowBuffer<T> &b) {
  std::swap(a.buf.ptr, b.buf.ptr);
  std::swap(a.buf.count, b.buf.count);
}

}  // namespace

Status gpu_index_edit(IndexStore *st, const IndexEdit &e, IndexAppendOut *out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = ensure_device();
  if (!s.ok()) return s;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != st->device) return Status::Make(NeedleError_InvalidArgument, "index: the current device is not the one the index was created on");
  st->used = true;
  if (e.n_old != st->n || e.n_new < 1 || e.regions < 1 || e.regions > 2)
    return Status::Make(NeedleError_InvalidArgument, "index edit: inconsistent sizes");
  hipStream_t stream = library_stream();
  const uint64_t buckets = edit_buckets(e), listed = (uint64_t)e.num_pairs * e.regions, rows = (uint64_t)e.n_new * e.regions;
  if (buckets >= 0xFFFFFFF0ull || e.total_hashes > UINT32_MAX || e.total_ts > UINT32_MAX)
    return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 hashes or sequence pairs");
  const uint64_t scan_len = std::max(buckets, listed);
  if (!(s = st->hash2.reserve(std::max<uint64_t>(e.total_hashes, 1), 0, stream)).ok() ||
      !(s = st->ts_table2.reserve(std::max<uint64_t>(e.total_ts, 1), 0, stream)).ok() ||
      !(s = st->row_len2.reserve(rows, 0, stream)).ok() || !(s = st->row_ts2.reserve(rows, 0, stream)).ok() ||
      !(s = st->row_seek2.reserve(rows, 0, stream)).ok() || !(s = st->hash_duration2.reserve(e.n_new, 0, stream)).ok() ||
      !(s = st->start2.reserve(buckets + 1, 0, stream)).ok() || !(s = st->valid2.reserve(std::max<uint64_t>(buckets, 1), 0, stream)).ok() ||
      !(s = st->src.reserve(std::max<uint64_t>(buckets, 1))).ok() || !(s = st->old_of_new.reserve(e.n_new)).ok() ||
      !(s = st->new_of_old.reserve(std::max<uint32_t>(e.n_old, 1))).ok() || !(s = st->gone.reserve(std::max<size_t>(e.num_gone, 1))).ok() ||
      !(s = st->pair_ids.reserve(std::max<size_t>(e.num_pairs, 1))).ok() ||
      !(s = st->segments.reserve(std::max<size_t>(e.num_hash_rows + e.num_ts_rows, 1))).ok() ||
      !(s = st->sums.reserve((scan_len + kScanBlock - 1) / kScanBlock + 1)).ok() || !(s = st->ctl.reserve(8)).ok() ||
      !(s = st->run_count.reserve(1)).ok() || !(s = st->flag.reserve(e.n_new)).ok() || !(s = st->list.reserve(e.n_new)).ok() ||
      !(s = st->results.reserve(e.n_new)).ok())
    return s;
  const size_t pinned_want = 16 + ((size_t)e.n_new + 2) * sizeof(uint32_t) + (size_t)e.n_new * sizeof(NeedleHipSearchResult);
  if (pinned_want > st->pinned_bytes) {
    if (st->pinned) (void)hipHostFree(st->pinned);
    st->pinned = nullptr;
    st->pinned_bytes = 0;
    NEEDLE_HIP_TRY(hipHostMalloc(&st->pinned, 2 * pinned_want, hipHostMallocDefault));
    st->pinned_bytes = 2 * pinned_want;
  }
  st->capacity = (uint32_t)std::min<uint64_t>(0x7fffffffu, std::max<uint64_t>(st->capacity, 3 * (uint64_t)e.num_problems));
  for (int attempt = 0; attempt < 2; attempt++) {
    const uint32_t capacity = st->capacity;
    const uint64_t entries1 = st->entries + capacity;  // the committed slots and this edit's; the rebuilt store holds at most as many
    if (entries1 >= 0xFFFFFFF0ull) return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 heap entries");
    const uint64_t cand = 2 * entries1;
    if (!(s = st->entry.reserve(entries1, st->entries, stream)).ok() || !(s = st->entry2.reserve(entries1, 0, stream)).ok() ||
        !(s = st->runs.reserve(capacity)).ok() || !(s = st->sorted.reserve(capacity)).ok() ||
        !(s = st->count.reserve(std::max<uint64_t>(listed, 1))).ok() || !(s = st->fill.reserve(std::max<uint64_t>(listed, 1))).ok() ||
        !(s = st->lstart.reserve(listed + 1)).ok() || !(s = st->lvalid.reserve(std::max<uint64_t>(listed, 1))).ok() ||
        !(s = st->large_list.reserve(capacity / (kEpilogueBucketLimit + 1) + 1)).ok() || !(s = st->cand.reserve(cand)).ok() ||
        !(s = st->links.reserve(cand)).ok())
      return s;
    if (!st->listed_attr_set) {
      NEEDLE_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pair_entries_large_kernel<ListedPairs, const uint32_t *>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kEpilogueLargeLimit * sizeof(unsigned long long))));
      st->listed_attr_set = true;
    }
    if (!(s = index_edit_tables(st, e, capacity, stream)).ok() || !(s = index_edit_rebuild(st, e, stream, out)).ok()) return s;
    if (out->found <= capacity) {
      out->runs.clear();
      if ((out->failed & kEpilogueBucketTooLarge) && out->found) {  // the host computes the listed pairs' entries (index.cpp)
        out->runs.resize(out->found);
        NEEDLE_HIP_TRY(hipMemcpy(out->runs.data(), st->runs.ptr, (size_t)out->found * sizeof(NeedleHipRun), hipMemcpyDeviceToHost));
      }
      return Status::Ok();
    }
    st->capacity = out->found;  // the scan is deterministic: a second pass with the exact size fits
  }
  return Status::Make(NeedleError_Unknown, "index edit: run list did not fit after resize");
}

Status gpu_index_edit_host_entries(IndexStore *st, const IndexEdit &e, const std::vector<uint32_t> &start, const std::vector<uint32_t> &valid,
                                   const std::vector<IndexEntry> &entries, IndexAppendOut *out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  hipStream_t stream = library_stream();
  const uint64_t listed = (uint64_t)e.num_pairs * e.regions;
  if (start.size() != listed || valid.size() != listed || st->entries + entries.size() > st->entry.buf.count || listed > st->lvalid.count)
    return Status::Make(NeedleError_InvalidArgument, "index edit: host entries do not fit the edit");
  if (!entries.empty())
    NEEDLE_HIP_TRY(hipMemcpyAsync(st->entry.ptr() + st->entries, entries.data(), entries.size() * sizeof(IndexEntry), hipMemcpyHostToDevice, stream));
  if (listed) {
    NEEDLE_HIP_TRY(hipMemcpyAsync(st->lstart.ptr, start.data(), listed * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    NEEDLE_HIP_TRY(hipMemcpyAsync(st->lvalid.ptr, valid.data(), listed * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  }
  NEEDLE_HIP_TRY(hipMemsetAsync(st->ctl.ptr + 2, 0, sizeof(uint32_t), stream));  // the failure word
  const uint32_t found = out->found;
  Status s = index_edit_rebuild(st, e, stream, out);
  out->found = found;
  return s;
}

void index_store_switch(IndexStore *st, const IndexEdit &e, uint32_t held) {
  swap_buffers(st->entry, st->entry2);
  swap_buffers(st->start, st->start2);
  swap_buffers(st->valid, st->valid2);
  swap_buffers(st->row_len, st->row_len2);
  swap_buffers(st->row_ts, st->row_ts2);
  swap_buffers(st->hash, st->hash2);
  swap_buffers(st->row_seek, st->row_seek2);
  swap_buffers(st->ts_table, st->ts_table2);
  swap_buffers(st->hash_duration, st->hash_duration2);
  st->n = e.n_new;
  st->buckets = edit_buckets(e);
  st->entries = held;
  st->rows = (uint64_t)e.n_new * e.regions;
  st->ts = e.total_ts;
  st->hashes = e.total_hashes;
}

void index_store_clear(IndexStore *st) {
  st->n = 0;
  st->buckets = st->entries = st->rows = st->ts = st->hashes = 0;
}

Status index_store_sizes(IndexStore *st, uint64_t sizes[4]) {
  sizes[0] = 0;
  sizes[1] = st->entries;
  sizes[2] = st->hashes;
  sizes[3] = st->ts;
  if (!st->buckets) return Status::Ok();
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != st->device) return Status::Make(NeedleError_InvalidArgument, "index: the current device is not the one the index was created on");
  std::vector<uint32_t> valid(st->buckets);
  hipStream_t stream = library_stream();
  NEEDLE_HIP_TRY(hipMemcpyAsync(valid.data(), st->valid.ptr(), valid.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  for (uint32_t v : valid) sizes[0] += v;
  return Status::Ok();
}

}  // namespace needle
