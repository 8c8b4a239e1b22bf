// The device code of the per-video epilogue that its two users share -- the library job (epilogue.hip, which says what
// each kernel computes) and the incremental index's store (index_store.hip) -- and the host helpers that launch it.
// Included by the .hip that launches the kernels, like scan_mfma_kernel.h.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <set>

#include "../../include/needle_hip.h"
#include "epilogue.h"
#include "hipctx.h"
#include "pair_ids.h"

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
struct GroupedPairs {  // a library of seasons: problem / regions = a grouped pair id (pair_ids.h), the tables in device memory
  GroupView groups;
  __device__ GroupedPairs(const EpilogueParams &, const GroupView &g) : groups(g) {}
  // once per bucket that has runs: a bisection over the groups' bases, then over the group's rows.  (The buckets are sized
  // by the same tables, so every bucket is a pair; were one not, it reads video 0's rows, inside the tables.)
  __device__ void at(uint64_t p, uint32_t *i, uint32_t *j) const {
    if (!grouped_pair_at(groups, p, i, j)) *i = *j = 0;
  }
};
// The grouped index (pair_ids.h IndexGroupView: append-stable ids, the tables in device memory).  An append: problem / regions
// = id - first, first = the append's first new id.  Once per bucket that has runs: a bisection over the videos' vbase.  (The
// buckets are sized by the same tables, so every bucket is a pair; were one not, it reads video 0's rows, inside the tables.)
struct IndexGroupAppendPairs {
  IndexGroupView groups;
  uint64_t first;
  __device__ IndexGroupAppendPairs(const EpilogueParams &, const IndexGroupView &g, uint64_t first_pair) : groups(g), first(first_pair) {}
  __device__ void at(uint64_t p, uint32_t *i, uint32_t *j) const {
    if (!index_group_pair_at(groups, first + p, i, j)) *i = *j = 0;
  }
};
struct IndexGroupListedPairs {  // an edit of the grouped index: table[listed] = the pair's id in the rebuilt store
  IndexGroupView groups;
  const uint32_t *table;
  __device__ IndexGroupListedPairs(const EpilogueParams &, const IndexGroupView &g, const uint32_t *pair_ids) : groups(g), table(pair_ids) {}
  __device__ void at(uint64_t p, uint32_t *i, uint32_t *j) const {
    if (!index_group_pair_at(groups, table[p], i, j)) *i = *j = 0;
  }
};

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
// winners_out: what the selection knows beside the result; only EvidenceVideos keeps it.
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
  __device__ uint32_t slots(const EpilogueParams &pr, uint32_t) const { return pr.n - 1; }
  __device__ bool is_source(uint32_t q, uint32_t v) const { return q >= v; }
  __device__ uint32_t partner(uint32_t q, uint32_t v) const { return q < v ? q : q + 1; }
  __device__ uint64_t video_hash_duration(uint32_t) const { return hash_duration; }
  __device__ void winners_out(uint32_t, unsigned long long, uint32_t, const BestKey &, const BestKey &, bool, const uint32_t *) const {}  // (EvidenceVideos')
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
  __device__ uint32_t slots(const EpilogueParams &pr, uint32_t) const { return pr.n - 1; }
  __device__ bool is_source(uint32_t q, uint32_t v) const { return q >= v; }
  __device__ uint32_t partner(uint32_t q, uint32_t v) const { return q < v ? q : q + 1; }
  __device__ uint64_t video_hash_duration(uint32_t v) const { return hash_durations[v]; }
  __device__ void winners_out(uint32_t, unsigned long long, uint32_t, const BestKey &, const BestKey &, bool, const uint32_t *) const {}
};
// What find_best_match knows about its winners and throws away, per video: left for match_evidence_kernel.
struct DeviceWinners {
  unsigned long long pool_base;  // the video's candidates in the pool, `candidates` of them
  uint32_t candidates, pad;
  struct {
    uint32_t have, index, support;  // the winner's candidate index and its links (`count` of :466)
    float weighted;                 // count * 0.3 + secs * 0.7 (:469, before the negation)
  } region[2];                      // [0] opening, [1] ending
};
struct EvidenceVideos {  // the index's evidence: EVERY video of the store, buckets as IndexVideos, results[v], and the winners written out
  const uint64_t *hash_durations;
  DeviceWinners *winners;  // zeroed by the host: a video without candidates writes nothing
  __device__ EvidenceVideos(const EpilogueParams &, const uint64_t *hd, DeviceWinners *w) : hash_durations(hd), winners(w) {}
  __device__ bool live(uint32_t) const { return true; }
  __device__ uint32_t video(uint32_t block) const { return block; }
  __device__ uint64_t pair(uint32_t q, uint32_t v) const { return q < v ? column_start(v) + q : column_start(q + 1) + v; }
  __device__ uint32_t out(uint32_t, uint32_t v) const { return v; }
  __device__ uint32_t slots(const EpilogueParams &pr, uint32_t) const { return pr.n - 1; }
  __device__ bool is_source(uint32_t q, uint32_t v) const { return q >= v; }
  __device__ uint32_t partner(uint32_t q, uint32_t v) const { return q < v ? q : q + 1; }
  __device__ uint64_t video_hash_duration(uint32_t v) const { return hash_durations[v]; }
  // thread 0, behind the selection: where the video's c candidates are, and each region's winner with its links
  __device__ void winners_out(uint32_t v, unsigned long long pool_base, uint32_t c, const BestKey &opening, const BestKey &ending,
                              bool include_endings, const uint32_t *links) const {
    DeviceWinners w;
    w.pool_base = pool_base;
    w.candidates = c;
    w.pad = 0;
    for (int which = 0; which < 2; which++) {
      const BestKey &k = which == 0 ? opening : ending;
      const bool have = k.have && (which == 0 || include_endings);  // :486
      w.region[which].have = have ? 1u : 0u;
      w.region[which].index = have ? k.index : 0u;
      w.region[which].support = have ? links[k.index] : 0u;
      w.region[which].weighted = have ? -k.score : 0.f;
    }
    winners[v] = w;
  }
};

// A library of seasons: EVERY video is a workgroup, its pairs are its group's -- size - 1 slots, none for a video alone in its
// group, which writes "no result" -- buckets in the grouped pair order (pair_ids.h), results[v].  The workgroup's video is
// its block, so what the slot passes need of the tables (rank, group size, base) is read once, at addresses every lane
// shares: scalar loads into scalar registers, and a slot's pair id is arithmetic on them -- the member list is not read here.
// A job of several ranks takes a block of the videos: workgroup b is video pr.v0 + b (pr.v0 = 0 where all videos are wanted),
// and writes results[v] all the same.
struct GroupedVideos {
  uint64_t base;
  uint32_t rank, size, v0;
  const uint64_t *hash_durations;
  __device__ GroupedVideos(const EpilogueParams &pr, const GroupView &g, const uint64_t *hd) : v0(pr.v0), hash_durations(hd) {
    const uint32_t v = pr.v0 + blockIdx.x;
    const uint32_t group = g.group_of[v];
    rank = g.rank_of[v];
    size = g.size[group];
    base = g.base[group];
  }
  __device__ bool live(uint32_t) const { return true; }
  __device__ uint32_t video(uint32_t block) const { return v0 + block; }
  __device__ uint64_t pair(uint32_t q, uint32_t) const { return grouped_rank_slot_pair(base, rank, size, q); }
  __device__ uint32_t out(uint32_t, uint32_t v) const { return v; }
  __device__ uint32_t slots(const EpilogueParams &, uint32_t) const { return size - 1; }
  __device__ bool is_source(uint32_t q, uint32_t) const { return q >= rank; }  // slot q is (lower member, v) below v's rank
  __device__ uint64_t video_hash_duration(uint32_t v) const { return hash_durations[v]; }
  __device__ void winners_out(uint32_t, unsigned long long, uint32_t, const BestKey &, const BestKey &, bool, const uint32_t *) const {}
};

// The grouped index: what a workgroup's video needs of the tables (pair_ids.h IndexGroupView) -- rank, group size, its own vbase,
// where its group's members start -- read once, at addresses every lane shares.  Slot q below the rank is (q-th member, v), in
// v's own column: arithmetic.  A slot at or above it is (v, member q + 1), in that member's column: one read of the member
// list and one of that member's vbase.  A video alone in its group has no slot and writes "no result".
struct IndexGroupSlots {
  const uint32_t *members;  // the video's group's
  const uint64_t *vbase;
  uint64_t own;             // vbase[v]
  uint32_t rank, size;
  __device__ void load(const IndexGroupView &g, uint32_t v) {
    const uint32_t group = g.group_of[v];
    rank = g.rank_of[v];
    size = g.size[group];
    members = g.members + g.first[group];
    vbase = g.vbase;
    own = g.vbase[v];
  }
  __device__ void none() {
    members = nullptr;
    vbase = nullptr;
    own = 0;
    rank = 0;
    size = 1;
  }
  __device__ uint64_t pair(uint32_t q) const { return q < rank ? own + q : vbase[members[q + 1]] + rank; }
  __device__ uint32_t partner(uint32_t q) const { return members[q < rank ? q : q + 1]; }
};
struct IndexGroupVideos {  // an append or an edit: the videos listed (*count of them), results[block] -- IndexVideos' grouped counterpart
  IndexGroupSlots slot;
  const uint32_t *list, *count;
  const uint64_t *hash_durations;
  __device__ IndexGroupVideos(const EpilogueParams &, const IndexGroupView &g, const uint32_t *l, const uint32_t *c, const uint64_t *hd)
      : list(l), count(c), hash_durations(hd) {
    if (blockIdx.x < *c) slot.load(g, l[blockIdx.x]);  // (a workgroup beyond the list returns at once: nothing of the tables is read)
    else slot.none();
  }
  __device__ bool live(uint32_t block) const { return block < *count; }
  __device__ uint32_t video(uint32_t block) const { return list[block]; }
  __device__ uint64_t pair(uint32_t q, uint32_t) const { return slot.pair(q); }
  __device__ uint32_t out(uint32_t block, uint32_t) const { return block; }
  __device__ uint32_t slots(const EpilogueParams &, uint32_t) const { return slot.size - 1; }
  __device__ bool is_source(uint32_t q, uint32_t) const { return q >= slot.rank; }
  __device__ uint32_t partner(uint32_t q, uint32_t) const { return slot.partner(q); }
  __device__ uint64_t video_hash_duration(uint32_t v) const { return hash_durations[v]; }
  __device__ void winners_out(uint32_t, unsigned long long, uint32_t, const BestKey &, const BestKey &, bool, const uint32_t *) const {}
};
struct IndexGroupEvidenceVideos {  // the grouped index's evidence: EVERY video, its group's slots, results[v], the winners written out
  IndexGroupSlots slot;
  const uint64_t *hash_durations;
  DeviceWinners *winners;  // zeroed by the host: a video without candidates writes nothing
  __device__ IndexGroupEvidenceVideos(const EpilogueParams &, const IndexGroupView &g, const uint64_t *hd, DeviceWinners *w)
      : hash_durations(hd), winners(w) {
    if (blockIdx.x < g.videos) slot.load(g, blockIdx.x);
    else slot.none();
  }
  __device__ bool live(uint32_t) const { return true; }
  __device__ uint32_t video(uint32_t block) const { return block; }
  __device__ uint64_t pair(uint32_t q, uint32_t) const { return slot.pair(q); }
  __device__ uint32_t out(uint32_t, uint32_t v) const { return v; }
  __device__ uint32_t slots(const EpilogueParams &, uint32_t) const { return slot.size - 1; }
  __device__ bool is_source(uint32_t q, uint32_t) const { return q >= slot.rank; }
  __device__ uint32_t partner(uint32_t q, uint32_t) const { return slot.partner(q); }
  __device__ uint64_t video_hash_duration(uint32_t v) const { return hash_durations[v]; }
  // as EvidenceVideos' (a function of its own: that one stays the single caller's it was, and its kernel's code what it was)
  __device__ void winners_out(uint32_t v, unsigned long long pool_base, uint32_t c, const BestKey &opening, const BestKey &ending,
                              bool include_endings, const uint32_t *links) const {
    DeviceWinners w;
    w.pool_base = pool_base;
    w.candidates = c;
    w.pad = 0;
    for (int which = 0; which < 2; which++) {
      const BestKey &k = which == 0 ? opening : ending;
      const bool have = k.have && (which == 0 || include_endings);  // :486
      w.region[which].have = have ? 1u : 0u;
      w.region[which].index = have ? k.index : 0u;
      w.region[which].support = have ? links[k.index] : 0u;
      w.region[which].weighted = have ? -k.score : 0.f;
    }
    winners[v] = w;
  }
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
  const uint32_t slots = videos.slots(pr, v);  // the video's pairs in lexicographic order: (q, v) for q < v, then (v, q + 1)
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
    if (cnt && cnt <= kOwnCopy) copy_entries(b, videos.is_source(q, v), at, 0u, 1u);
    __syncthreads();
    for (uint32_t qq = 0; qq < 256; qq++) {
      if (slot_cnt[qq] <= kOwnCopy) continue;  // (uniform)
      const uint32_t q2 = base + qq;
      copy_entries(bucket_of(q2), videos.is_source(q2, v), slot_at[qq], t, 256u);
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
    videos.winners_out(v, pool_base, c, best[0][0], best[1][0], pr.include_endings != 0, links);  // (EvidenceVideos only)
    if (bad) atomicAdd(failed, 1u);
    results[videos.out(blockIdx.x, v)] = res;
  }
}

// The evidence of the index's results (needle_hip.h NeedleHipSearchEvidence): one workgroup per video, behind
// best_match_kernel<EvidenceVideos> on the same stream, whose winners (candidate index, links, score) and candidate pool it
// reads.  It walks the video's pair slots in the reference's order, 256 at a time, with the prefix sums of their candidate
// counts, as best_match's pass 2 does: the slot whose range holds a winner's index gives the partner and the role, the offset
// in it the region and the DeviceEntry with both intervals and both simhashes.  On the same walk a slot counts as a partner of
// a winner if any of its candidates is within the bound of the winner's hash (both regions, :436-453): its own lane looks while
// the candidates are few, the workgroup where a slot holds many (a pair of silent stretches).  Any number of slots and of
// candidates: nothing here is staged by candidate.
template <class Videos, class... Extra>
__global__ __launch_bounds__(256) void match_evidence_kernel(EpilogueParams pr, const uint32_t *__restrict__ start,
                                                             const uint32_t *__restrict__ valid, const DeviceEntry *__restrict__ entries,
                                                             const Candidate *__restrict__ cand_pool,
                                                             NeedleHipSearchEvidence *__restrict__ out, Extra... extra) {
  __shared__ uint32_t scan[256];
  __shared__ uint32_t carry;
  __shared__ uint32_t slot_cnt[256], slot_at[256], slot_near[256];
  __shared__ uint32_t partners[2];
  __shared__ NeedleHipSearchEvidence rec;
  const uint32_t v = blockIdx.x, t = threadIdx.x;
  if (v >= pr.n) return;
  const Videos videos(pr, extra...);  // (the policy of the launch in front: the same slots, its winners)
  const DeviceWinners w = videos.winners[v];
  if (t == 0) {
    memset(&rec, 0, sizeof(rec));
    rec.opening.partner = rec.ending.partner = 0xFFFFFFFFu;
    carry = 0;
    partners[0] = partners[1] = 0;
  }
  __syncthreads();
  bool have[2];
  uint32_t hash[2];
  const Candidate *cand = cand_pool + w.pool_base;
  for (int which = 0; which < 2; which++) {
    have[which] = w.region[which].have && w.region[which].index < w.candidates;
    hash[which] = have[which] ? cand[w.region[which].index].hash : 0u;
  }
  if (!have[0] && !have[1]) {  // no candidate at all, or none of either kind (uniform)
    if (t == 0) out[v] = rec;
    return;
  }
  const uint32_t slots = videos.slots(pr, v);  // (q, v) for q < v, then (v, q + 1); a grouped index: the video's group's
  auto bucket_of = [&](uint32_t q) -> uint64_t { return videos.pair(q, v) * pr.regions; };
  auto near_of = [&](uint32_t h) -> uint32_t {
    return (have[0] && (uint32_t)__popc(h ^ hash[0]) < pr.bound ? 1u : 0u) | (have[1] && (uint32_t)__popc(h ^ hash[1]) < pr.bound ? 2u : 0u);
  };
  constexpr uint32_t kOwnLook = 16;
  for (uint32_t base = 0; base < slots; base += 256) {
    const uint32_t q = base + t;
    uint32_t cnt = 0, openings = 0;
    uint64_t b = 0;
    if (q < slots) {
      b = bucket_of(q);
      openings = valid[b];
      cnt = openings + (pr.regions == 2 ? valid[b + 1] : 0u);
    }
    scan[t] = cnt;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const uint32_t add = (int)t >= d ? scan[t - d] : 0u;
      __syncthreads();
      scan[t] += add;
      __syncthreads();
    }
    const uint32_t at = carry + scan[t] - cnt;
    for (int which = 0; which < 2; which++) {
      const uint32_t index = w.region[which].index;
      if (!have[which] || index < at || index - at >= cnt) continue;
      uint32_t k = index - at;  // openings first, then endings (:414-431)
      const uint32_t r = k < openings ? 0u : 1u;
      if (r) k -= openings;
      const DeviceEntry e = entries[start[b + r] + k];
      const bool as_source = videos.is_source(q, v);
      NeedleHipMatchEvidence &ev = which == 0 ? rec.opening : rec.ending;
      ev.partner = videos.partner(q, v);
      ev.is_source = as_source ? 1u : 0u;
      ev.match_hash = as_source ? e.src_hash : e.dst_hash;
      ev.partner_hash = as_source ? e.dst_hash : e.src_hash;
      ev.start_ns = as_source ? e.src_start : e.dst_start;
      ev.end_ns = as_source ? e.src_end : e.dst_end;
      ev.partner_start_ns = as_source ? e.dst_start : e.src_start;
      ev.partner_end_ns = as_source ? e.dst_end : e.src_end;
    }
    uint32_t near = 0;
    if (cnt <= kOwnLook)
      for (uint32_t k = 0; k < cnt; k++) near |= near_of(cand[at + k].hash);
    slot_cnt[t] = cnt;
    slot_at[t] = at;
    slot_near[t] = near;
    __syncthreads();
    for (uint32_t qq = 0; qq < 256; qq++) {
      const uint32_t many = slot_cnt[qq];
      if (many <= kOwnLook) continue;  // (uniform)
      uint32_t mine = 0;
      for (uint32_t k = t; k < many; k += 256) mine |= near_of(cand[slot_at[qq] + k].hash);
      if (mine) atomicOr(&slot_near[qq], mine);
    }
    __syncthreads();
    near = slot_near[t];
    const unsigned long long near0 = __ballot(near & 1u), near1 = __ballot(near & 2u);
    if ((t & 63u) == 0) {
      if (near0) atomicAdd(&partners[0], (uint32_t)__popcll(near0));
      if (near1) atomicAdd(&partners[1], (uint32_t)__popcll(near1));
    }
    if (t == 255) carry += scan[255];
    __syncthreads();
  }
  if (t == 0) {
    for (int which = 0; which < 2; which++) {
      if (!have[which]) continue;
      NeedleHipMatchEvidence &ev = which == 0 ? rec.opening : rec.ending;
      ev.candidate = w.region[which].index;
      ev.candidates = w.candidates;
      ev.support = w.region[which].support;
      ev.partners = partners[which];
      ev.score = w.region[which].weighted;
    }
    out[v] = rec;
  }
}

// ---- the host side of the entries pipeline: run list -> counting sort by bucket -> every bucket's heap entries ----------
// Shared by the library job (epilogue.hip) and the incremental index's append and edit (index_store.hip).  Everything is
// enqueued on the caller's stream; the callers hold gpu_mutex().

// The control words the kernels share, in device memory.  The kernels take the members' addresses; the layout is fixed.
struct EpilogueControl {
  unsigned long long cand_cursor;  // best_match_kernel: the next free slot of the candidate pool
  uint32_t failed;                 // videos whose padding / hash duration exceed the match end, | kEpilogueBucketTooLarge
  uint32_t large_count;            // buckets on pair_entries_large_kernel's list
  uint32_t listed;                 // (the index) videos listed for best_match_kernel
  uint32_t pad[3];
};
static_assert(sizeof(EpilogueControl) == 8 * sizeof(uint32_t) && offsetof(EpilogueControl, cand_cursor) == 0 &&
                  offsetof(EpilogueControl, failed) == 2 * sizeof(uint32_t) && offsetof(EpilogueControl, large_count) == 3 * sizeof(uint32_t) &&
                  offsetof(EpilogueControl, listed) == 4 * sizeof(uint32_t),
              "the control words' layout");

// What the pipeline needs beside its inputs and the entries it writes.
struct EntriesScratch {
  DeviceBuffer<uint32_t> count, fill, start, valid, sums, large_list;  // per bucket: start[buckets + 1]; valid = the heap's size
  DeviceBuffer<NeedleHipRun> sorted;
  static size_t sums_for(uint64_t n) { return (n + kScanBlock - 1) / kScanBlock + 1; }
  Status reserve(uint64_t buckets, uint64_t runs) {
    const size_t some = std::max<uint64_t>(buckets, 1);
    Status s;
    if (!(s = count.reserve(some)).ok() || !(s = fill.reserve(some)).ok() || !(s = start.reserve(buckets + 1)).ok() ||
        !(s = valid.reserve(some)).ok() || !(s = sums.reserve(sums_for(buckets))).ok() || !(s = sorted.reserve(runs)).ok() ||
        !(s = large_list.reserve(runs / (kEpilogueBucketLimit + 1) + 1)).ok())
      return s;
    return Status::Ok();
  }
};

// count[0..n) -> start[0..n], start[n] = the total (sums: EntriesScratch::sums_for(n) words)
inline void enqueue_exclusive_scan(const uint32_t *count, uint32_t n, uint32_t *sums, uint32_t *start, hipStream_t stream) {
  const uint32_t blocks = (uint32_t)(((uint64_t)n + kScanBlock - 1) / kScanBlock);
  hipLaunchKernelGGL(scan_block_sums_kernel, dim3(blocks), dim3(256), 0, stream, count, n, sums);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, sums, blocks);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(blocks), dim3(256), 0, stream, count, n, sums, start);
}

// The counting sort of the segments' runs (`max_runs` at most) by bucket into sc->sorted, sc->start; timed as `timer_name`.
inline Status enqueue_bucket_sort(const char *timer_name, const RunSegments &segs, uint32_t buckets, uint64_t max_runs, EntriesScratch *sc,
                                  hipStream_t stream) {
  NEEDLE_HIP_TRY(hipMemsetAsync(sc->count.ptr, 0, buckets * sizeof(uint32_t), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(sc->fill.ptr, 0, buckets * sizeof(uint32_t), stream));
  const uint32_t run_grid = (uint32_t)std::min<uint64_t>(4096, (max_runs + 255) / 256);
  KernelTimer timer(timer_name, stream);
  hipLaunchKernelGGL(bucket_count_kernel, dim3(run_grid), dim3(256), 0, stream, segs, buckets, sc->count.ptr);
  enqueue_exclusive_scan(sc->count.ptr, buckets, sc->sums.ptr, sc->start.ptr, stream);
  hipLaunchKernelGGL(bucket_scatter_kernel, dim3(run_grid), dim3(256), 0, stream, segs, buckets, sc->start.ptr, sc->fill.ptr, sc->sorted.ptr);
  return Status::Ok();
}

// The sorted buckets' heap entries into `entries` (at sc->start[b]), their sizes into sc->valid, under the pair numbering
// `Pairs` (its trailing kernel arguments: `extra`).  The caller opens the KernelTimer: an append times one more kernel with
// these.  pair_entries_large_kernel's LDS is beyond the default limit: the attribute that allows it is per function and per
// device, so each instantiation keeps the devices it has set it on.
template <class Pairs, class... Extra>
Status enqueue_pair_entries(int device, const EpilogueParams &pr, const EntriesScratch &sc, const uint32_t *row_len, const uint32_t *row_ts,
                            const uint64_t *row_seek, const uint64_t *ts, DeviceEntry *entries, EpilogueControl *ctl, hipStream_t stream,
                            Extra... extra) {
  constexpr size_t kLargeLds = kEpilogueLargeLimit * sizeof(unsigned long long);
  static std::set<int> lds_allowed;  // (under gpu_mutex)
  if (!lds_allowed.count(device)) {
    NEEDLE_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pair_entries_large_kernel<Pairs, Extra...>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLargeLds));
    lds_allowed.insert(device);
  }
  hipLaunchKernelGGL((pair_entries_kernel<Pairs, Extra...>), dim3((pr.buckets + 63) / 64), dim3(64), 0, stream, pr, sc.start.ptr, sc.sorted.ptr,
                     row_len, row_ts, row_seek, ts, entries, sc.valid.ptr, &ctl->failed, &ctl->large_count, sc.large_list.ptr, extra...);
  // the buckets one lane should not order (a stride loop over a list that is empty on ordinary audio: ~2 us then)
  hipLaunchKernelGGL((pair_entries_large_kernel<Pairs, Extra...>), dim3(512), dim3(256), kLargeLds, stream, pr, sc.start.ptr, sc.sorted.ptr, row_len,
                     row_ts, row_seek, ts, entries, sc.valid.ptr, &ctl->large_count, sc.large_list.ptr, extra...);
  return Status::Ok();
}

// EpilogueParams for `n` videos and `buckets` buckets, results for all of them, arena rows video * regions + region (the
// index's form; the library job sets its own v0, v1, rows_per_video and hash_duration).
inline EpilogueParams epilogue_params(const EpilogueOptions &o, bool large_ok, uint32_t n, uint64_t buckets) {
  EpilogueParams pr;
  std::memset(&pr, 0, sizeof(pr));
  pr.n = n;
  pr.regions = pr.rows_per_video = o.regions;
  pr.buckets = (uint32_t)buckets;
  pr.v1 = n;
  pr.bound = o.threshold + o.threshold / 2;
  pr.include_endings = o.include_endings ? 1u : 0u;
  pr.min_duration[0] = o.min_opening_duration;
  pr.min_duration[1] = o.min_ending_duration;
  pr.time_padding = o.time_padding;
  pr.large_ok = large_ok && getenv("NEEDLE_HIP_EPILOGUE_NO_LARGE") == nullptr ? 1u : 0u;  // (tests: the host fallback itself)
  return pr;
}

}  // namespace

}  // namespace needle
