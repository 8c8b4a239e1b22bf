// The device store of the incremental index (index.cpp says why keeping every pair's entries is enough): the heap entries
// of every pair searched so far and the tables that go with them, resident in HBM; an append searches the new pairs and
// adds theirs behind, an edit (removal / replacement) rebuilds the store under the new pair ids into a second set of
// tables.  The entries come from the library job's pipeline (epilogue_kernels.h) under the store's pair numberings.
// Nothing committed is written before index_store_commit / index_store_switch: an operation that fails leaves the store
// as it was.  A grouped index goes the same ways under pair_ids.h's grouped ids: its own policies of the entry
// and best-match kernels and grouped forms of the small kernels here; a plain index launches none of them.
// tests: test_gpu_index.py, test_gpu_index_edit.py, test_gpu_index_grouped.py.
#include <mutex>
#include <string>

#include "epilogue_kernels.h"
#include "index_store.h"
#include "pair_ids.h"

namespace needle {

namespace {

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

// ---- an append fed from a cross-matcher (gpu_index_append_matched) -------------------------------------------------------------
// The matcher's run list into the slab the scan of the new pairs would have left.  A run names its pair in the comparator's
// i-major order over all V videos; the store wants the column-major id less the append's first (pair_ids.h).  The scan's
// problems leave out a region one of whose rows can hold no run long enough (min_len 0) and apply max(min_len) of the two
// rows, where the matcher had one lower bound per region: those runs are dropped here.  A run that does not lie inside its
// two rows, or is not of a new pair, sets `error` and is dropped too, so nothing behind this reads outside a row.  The survivors
// of a wave leave together: one returning atomic per wave (stream_walk.h's push_runs).  A wave's 64 lanes take 64 consecutive
// runs, so every lane of a wave makes the same number of trips.
// A wave's survivors into the slab: one returning atomic per wave, a prefix count for the slots.  Every lane of the wave comes
// through here together.
__device__ __forceinline__ void ingest_push(const bool keep, const NeedleHipRun &run, NeedleHipRun *__restrict__ out, const uint32_t capacity,
                                            uint32_t *__restrict__ count) {
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
  if (mask == 0ull) return;
  uint32_t first = 0u;
  if (lane == 0u) first = atomicAdd(count, (uint32_t)__popcll(mask));
  first = (uint32_t)__builtin_amdgcn_readfirstlane((int)first);
  const uint32_t slot = first + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
  if (keep && slot < capacity) out[slot] = run;
}

// Pair (a, b, r) of an append onto n0 videos, b >= n0: whether `run` lies inside its two rows (else `error`), whether the scan's
// problems would have reported it, and its tag for the append.
__device__ __forceinline__ bool ingest_retag(NeedleHipRun &run, const uint32_t a, const uint32_t b, const uint32_t r, const uint32_t n0,
                                             const uint32_t regions, const uint32_t *__restrict__ min_len,
                                             const uint32_t *__restrict__ row_len, bool *good) {
  const uint64_t row_a = (uint64_t)a * regions + r, row_b = (uint64_t)b * regions + r;
  *good = run.src_end < row_len[row_a] && run.dst_end < row_len[row_b] && run.len <= min(run.src_end, run.dst_end);
  const uint32_t min_a = min_len[row_a], min_b = min_len[row_b];
  run.problem = (uint32_t)append_tag(a, b, r, n0, regions);
  return *good && min_a != 0u && min_b != 0u && run.len >= max(min_a, min_b);
}

__global__ __launch_bounds__(256) void index_ingest_runs_kernel(const NeedleHipRun *__restrict__ in, uint32_t num_runs, uint32_t videos,
                                                                uint32_t n0, uint32_t regions, const uint32_t *__restrict__ min_len,
                                                                const uint32_t *__restrict__ row_len, NeedleHipRun *__restrict__ out,
                                                                uint32_t capacity, uint32_t *__restrict__ count, uint32_t *__restrict__ error) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < num_runs; base += stride) {
    const uint64_t k = base + lane;
    bool keep = false;
    NeedleHipRun run{};
    if (k < num_runs) {
      run = in[k];
      uint32_t a = 0, b = 0, r = 0;
      bool good = decode_problem(run.problem, regions, videos, &a, &b, &r) && b >= n0;
      if (good) keep = ingest_retag(run, a, b, r, n0, regions, min_len, row_len, &good);
      if (!good) atomicOr(error, kIngestBadRun);
    }
    ingest_push(keep, run, out, capacity, count);
  }
}

// The grouped index's form: the list is a grouped cross-matcher's, whose runs name their pair by the grouped id over the V
// labels (`from`: pair_ids.h GroupView, base[] moves as groups grow), and the store wants the append-stable id (`to`:
// IndexGroupView) less the append's first.  Both views are over the same list, so they share every table but base / vbase.
// The same filter and the same kIngestBadRun rule: ingest_retag decides, and only the tag is replaced.
__global__ __launch_bounds__(256) void index_ingest_runs_grouped_kernel(const NeedleHipRun *__restrict__ in, uint32_t num_runs, GroupView from,
                                                                        IndexGroupView to, uint64_t first_pair, uint32_t n0, uint32_t regions,
                                                                        const uint32_t *__restrict__ min_len,
                                                                        const uint32_t *__restrict__ row_len, NeedleHipRun *__restrict__ out,
                                                                        uint32_t capacity, uint32_t *__restrict__ count,
                                                                        uint32_t *__restrict__ error) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < num_runs; base += stride) {
    const uint64_t k = base + lane;
    bool keep = false;
    NeedleHipRun run{};
    if (k < num_runs) {
      run = in[k];
      uint32_t a = 0, b = 0;
      const uint32_t r = run.problem % regions;
      uint64_t id = 0;
      bool good = grouped_pair_at(from, run.problem / regions, &a, &b) && b >= n0 && index_group_pair(to, a, b, &id) && id >= first_pair;
      if (good) {
        keep = ingest_retag(run, a, b, r, n0, regions, min_len, row_len, &good);
        run.problem = (uint32_t)((id - first_pair) * regions + r);
      }
      if (!good) atomicOr(error, kIngestBadRun);
    }
    ingest_push(keep, run, out, capacity, count);
  }
}

// ---- an append fed from a matcher made from the store and a cross-matcher over the arriving videos (gpu_index_append_streamed) --
// Both lists in one launch, the matcher's first.  A matcher run names its resident row (problem = resident * regions + region)
// and came from lane run_lane[q] = t * regions + region: pair (resident, n0 + t).  A cross-matcher run names its pair i-major
// over the k = n1 - n0 arriving videos alone: pair (n0 + a, n0 + b).  Everything else is index_ingest_runs_kernel.
__global__ __launch_bounds__(256) void index_ingest_streamed_kernel(const NeedleHipRun *__restrict__ in, uint32_t matcher_runs,
                                                                    uint32_t num_runs, const uint32_t *__restrict__ run_lane, uint32_t n0,
                                                                    uint32_t n1, uint32_t regions, const uint32_t *__restrict__ min_len,
                                                                    const uint32_t *__restrict__ row_len, NeedleHipRun *__restrict__ out,
                                                                    uint32_t capacity, uint32_t *__restrict__ count,
                                                                    uint32_t *__restrict__ error) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < num_runs; base += stride) {
    const uint64_t k = base + lane;
    bool keep = false;
    NeedleHipRun run{};
    if (k < num_runs) {
      run = in[k];
      uint32_t a = 0, b = 0, r = 0;
      bool good;
      if (k < matcher_runs) {
        const uint32_t from = run_lane[k];
        r = run.problem % regions;
        a = run.problem / regions;
        b = n0 + from / regions;
        good = a < n0 && b < n1 && from % regions == r;
      } else {
        good = decode_problem(run.problem, regions, n1 - n0, &a, &b, &r);
        a += n0;
        b += n0;
      }
      if (good) keep = ingest_retag(run, a, b, r, n0, regions, min_len, row_len, &good);
      if (!good) atomicOr(error, kIngestBadRun);
    }
    ingest_push(keep, run, out, capacity, count);
  }
}

// The new rows in the arena against the hashes their lanes were fed, each history with a device address of its own (a matcher's
// lanes are separate allocations): a workgroup per row.
__global__ __launch_bounds__(256) void index_compare_lanes_kernel(const IndexLaneRow *__restrict__ rows, uint32_t num_rows,
                                                                  const uint32_t *__restrict__ arena, uint32_t *__restrict__ error) {
  for (uint32_t s = blockIdx.x; s < num_rows; s += gridDim.x) {
    const IndexLaneRow g = rows[s];
    bool differ = false;
    for (uint64_t k = threadIdx.x; k < g.len; k += blockDim.x) differ = differ || arena[g.src + k] != g.history[k];
    if (differ) atomicOr(error, kIngestOtherHashes);
  }
}

// The new rows in the arena against the hashes their lanes were fed (the matcher's histories): a workgroup per row.
__global__ __launch_bounds__(256) void index_compare_rows_kernel(const IndexSegment *__restrict__ rows, uint32_t num_rows,
                                                                 const uint32_t *__restrict__ arena, const uint32_t *__restrict__ history,
                                                                 uint32_t *__restrict__ error) {
  for (uint32_t s = blockIdx.x; s < num_rows; s += gridDim.x) {
    const IndexSegment g = rows[s];
    bool differ = false;
    for (uint64_t k = threadIdx.x; k < g.len; k += blockDim.x) differ = differ || arena[g.src + k] != history[g.dst + k];
    if (differ) atomicOr(error, kIngestOtherHashes);
  }
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

// ---- the grouped index (pair_ids.h IndexGroupView): the kernels above that hard-wire the column-major id, under
// the grouped one.  index_edit_fresh_kernel reads its ids from the listed pairs' table and serves both.
// The videos whose candidate list a grouped append changed: the lower member i of a new pair (i, j) with an entry (old or
// arriving alike; every arriving video is listed anyway).  One bisection per bucket that has entries.
__global__ __launch_bounds__(256) void index_group_changed_kernel(uint32_t buckets, uint32_t regions, uint64_t first, IndexGroupView groups,
                                                                  const uint32_t *__restrict__ valid, uint32_t *__restrict__ flag) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < buckets; b += gridDim.x * blockDim.x) {
    if (valid[b] == 0) continue;
    uint32_t i, j;
    if (index_group_pair_at(groups, first + b / regions, &i, &j)) flag[i] = 1u;
  }
}
// A kept pair's new bucket -> its old bucket: the pair under the new tables, its two videos' old positions, their id under the
// old tables (removal keeps the relative order and the labels, so the two are of one old group with the same roles).
__global__ __launch_bounds__(256) void index_group_edit_buckets_kernel(uint32_t buckets, uint32_t regions, IndexGroupView groups,
                                                                       IndexGroupView old_groups, const uint32_t *__restrict__ old_of_new,
                                                                       const uint32_t *__restrict__ old_start,
                                                                       const uint32_t *__restrict__ old_valid, uint32_t *__restrict__ src,
                                                                       uint32_t *__restrict__ count) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < buckets; b += gridDim.x * blockDim.x) {
    uint32_t i, j;
    if (!index_group_pair_at(groups, b / regions, &i, &j)) continue;
    const uint32_t oi = old_of_new[i], oj = old_of_new[j];
    if (oi == kIndexFresh || oj == kIndexFresh) continue;
    uint64_t op;
    if (!index_group_pair(old_groups, oi, oj, &op)) continue;
    const uint64_t ob = op * regions + b % regions;
    src[b] = old_start[ob];
    count[b] = old_valid[ob];
  }
}
// Every kept video with an entry in a pair of a video removed or replaced: the committed store, old ids, the gone video's group only.
__global__ __launch_bounds__(256) void index_group_gone_partners_kernel(uint32_t n_old, uint32_t regions, IndexGroupView old_groups,
                                                                        const uint32_t *__restrict__ gone, uint32_t num_gone,
                                                                        const uint32_t *__restrict__ valid,
                                                                        const uint32_t *__restrict__ new_of_old, uint32_t *__restrict__ flag) {
  const uint64_t total = (uint64_t)num_gone * n_old;
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t x = gone[t / n_old], q = (uint32_t)(t % n_old);
    if (q == x || new_of_old[q] == kIndexFresh) continue;
    uint64_t p;
    if (!index_group_pair(old_groups, min(q, x), max(q, x), &p)) continue;  // (of another group: no pair)
    bool any = false;
    for (uint32_t r = 0; r < regions; r++) any = any || valid[p * regions + r] != 0;
    if (any) flag[new_of_old[q]] = 1u;
  }
}
// ... and every video with an entry in a listed pair
__global__ __launch_bounds__(256) void index_group_fresh_partners_kernel(uint32_t listed, uint32_t regions, IndexGroupView groups,
                                                                         const uint32_t *__restrict__ pair_ids,
                                                                         const uint32_t *__restrict__ lvalid, uint32_t *__restrict__ flag) {
  for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < listed; l += gridDim.x * blockDim.x) {
    if (lvalid[l] == 0) continue;
    uint32_t i, j;
    if (!index_group_pair_at(groups, pair_ids[l / regions], &i, &j)) continue;
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

// Every resident table of the store.  The store holds two sets: the current one, and the one an edit gathers the rebuilt
// store into.
struct StoreTables {
  GrowBuffer<DeviceEntry> entry;  // the per-pair entries and, per bucket b = p(i, j) * regions + r, where they start and how many
  GrowBuffer<uint32_t> start, valid, row_len, row_ts, hash;
  GrowBuffer<uint64_t> row_seek, ts_table, hash_duration;
};

// A grouped index's tables on the device (pair_ids.h IndexGroupView): the 32-bit ones in one buffer -- group_of[n], rank_of[n],
// members[n], size[groups], first[groups] -- and vbase[n + 1].  The store holds two: the committed list's, and the one an
// operation uploads the new list's into (committed with everything else).
struct DeviceGroupTables {
  DeviceBuffer<uint32_t> words;
  DeviceBuffer<uint64_t> vbase;
  IndexGroupView view{};
};

struct PinnedHead {  // what an operation reads back, in pinned memory: followed by list[n] and results[n]
  uint32_t found, failed, listed, held;
};
static_assert(sizeof(PinnedHead) == 16 && offsetof(PinnedHead, held) == 12, "four words before the list");

}  // namespace

struct IndexStore {
  // committed: what the index holds (an append that fails leaves these, and what lies below them, as they were)
  uint32_t n = 0;
  uint64_t buckets = 0, entries = 0, rows = 0, ts = 0, hashes = 0;
  StoreTables tables[2];
  StoreTables *cur = &tables[0], *next = &tables[1];  // (index_store_switch swaps the two)
  DeviceGroupTables group_tables[2];  // a grouped index's: [group_cur] the committed list's, the other an operation's
  int group_cur = 0;
  DeviceBuffer<uint32_t> src, old_of_new, new_of_old, gone, pair_ids;  // an edit's maps
  DeviceBuffer<IndexSegment> segments;
  // an operation's scratch
  EntriesScratch scratch;  // over the new (an append) or the listed (an edit) pairs' buckets
  DeviceBuffer<EpilogueControl> ctl;
  DeviceBuffer<uint32_t> flag, list, links, run_count;
  DeviceBuffer<NeedleHipRun> runs, matched_runs;  // the run list; a matcher's, as uploaded
  DeviceBuffer<uint32_t> matched_min_len, matched_error, run_lane;
  DeviceBuffer<uint64_t> matched_base;  // a grouped matcher's list: base[] of pair_ids.h GroupView over the operation's list
  DeviceBuffer<IndexLaneRow> lane_rows;
  DeviceBuffer<Candidate> cand;
  DeviceBuffer<NeedleHipSearchResult> results;
  PinnedHead *pinned = nullptr;
  size_t pinned_bytes = 0;
  // gpu_index_evidence's own: the winners best_match leaves, the records, and where they are read back
  DeviceBuffer<DeviceWinners> winners;
  DeviceBuffer<NeedleHipSearchEvidence> evidence;
  NeedleHipSearchEvidence *evidence_pinned = nullptr;
  size_t evidence_pinned_count = 0;
  uint32_t capacity = 1u << 16;  // of the run list; grows to what an append found
  bool used = false;  // an append has enqueued work (a store made without a device never has)
  int device = 0;
  ~IndexStore() {
    if (pinned) (void)hipHostFree(pinned);
    if (evidence_pinned) (void)hipHostFree(evidence_pinned);
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

uint64_t append_first_pair(const IndexAppend &a) { return a.groups ? a.groups->vbase[a.n0] : (uint64_t)a.n0 * (a.n0 - (a.n0 ? 1 : 0)) / 2; }
uint64_t append_buckets(const IndexAppend &a) {
  return ((a.groups ? a.groups->pairs() : (uint64_t)a.n1 * (a.n1 - 1) / 2) - append_first_pair(a)) * a.regions;
}
uint64_t edit_buckets(const IndexEdit &e) {
  return (e.groups ? e.groups->pairs() : (uint64_t)e.n_new * (e.n_new ? e.n_new - 1 : 0) / 2) * e.regions;
}

template <class T>
hipError_t upload(T *dst, const T *src, size_t count, hipStream_t stream) {  // (pageable source: staged before the call returns)
  return count ? hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, stream) : hipSuccess;
}

// A grouped operation's tables (the list after it) into the store's spare set: not the committed ones, which an edit reads
// beside them and a failing operation keeps.
Status index_upload_groups(IndexStore *st, const IndexGroupTables &g, hipStream_t stream) {
  DeviceGroupTables &d = st->group_tables[1 - st->group_cur];
  const size_t n = g.group_of.size(), groups = g.size.size();
  Status s;
  if (!(s = d.words.reserve(std::max<size_t>(3 * n + 2 * groups, 1))).ok() || !(s = d.vbase.reserve(n + 1)).ok()) return s;
  uint32_t *w = d.words.ptr;
  NEEDLE_HIP_TRY(upload(w, g.group_of.data(), n, stream));
  NEEDLE_HIP_TRY(upload(w + n, g.rank_of.data(), n, stream));
  NEEDLE_HIP_TRY(upload(w + 2 * n, g.members.data(), n, stream));
  NEEDLE_HIP_TRY(upload(w + 3 * n, g.size.data(), groups, stream));
  NEEDLE_HIP_TRY(upload(w + 3 * n + groups, g.first.data(), groups, stream));
  NEEDLE_HIP_TRY(upload(d.vbase.ptr, g.vbase.data(), n + 1, stream));
  d.view = IndexGroupView{w, w + n, w + 3 * n, w + 3 * n + groups, w + 2 * n, d.vbase.ptr, (uint32_t)n};
  return Status::Ok();
}
const IndexGroupView &operation_groups(const IndexStore *st) { return st->group_tables[1 - st->group_cur].view; }
const IndexGroupView &committed_groups(const IndexStore *st) { return st->group_tables[st->group_cur].view; }

Status index_check_device(const IndexStore *st) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != st->device) return Status::Make(NeedleError_InvalidArgument, "index: the current device is not the one the index was created on");
  return Status::Ok();
}

// how an append and an edit begin
Status index_enter(IndexStore *st) {
  Status s = ensure_device();
  if (!s.ok() || !(s = index_check_device(st)).ok()) return s;
  st->used = true;
  return Status::Ok();
}

// An operation's device work, which needs a capacity for the run list of its scan: enqueue(capacity, entry slots) is
// given the store's, and once more the exact one if the scan found more.  Sizes what both operations use: the results
// of up to `n` videos, the pipeline's scratch over `scratch_buckets` buckets, room for `capacity` new entries behind the
// committed ones.  With kEpilogueBucketTooLarge, out->runs is the run list, for the host (index.cpp).
template <class Enqueue>
Status index_run(IndexStore *st, const char *what, size_t num_problems, uint64_t scratch_buckets, uint32_t n, hipStream_t stream,
                 IndexAppendOut *out, Enqueue enqueue) {
  Status s;
  if (!(s = st->ctl.reserve(1)).ok() || !(s = st->run_count.reserve(1)).ok() || !(s = st->flag.reserve(n)).ok() ||
      !(s = st->list.reserve(n)).ok() || !(s = st->results.reserve(n)).ok())
    return s;
  const size_t pinned_want = sizeof(PinnedHead) + ((size_t)n + 2) * sizeof(uint32_t) + (size_t)n * sizeof(NeedleHipSearchResult);
  if (pinned_want > st->pinned_bytes) {
    if (st->pinned) (void)hipHostFree(st->pinned);
    st->pinned = nullptr;
    st->pinned_bytes = 0;
    NEEDLE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&st->pinned), 2 * pinned_want, hipHostMallocDefault));
    st->pinned_bytes = 2 * pinned_want;
  }
  st->capacity = (uint32_t)std::min<uint64_t>(0x7fffffffu, std::max<uint64_t>(st->capacity, 3 * (uint64_t)num_problems));
  for (int attempt = 0; attempt < 2; attempt++) {
    const uint32_t capacity = st->capacity;
    const uint64_t entries1 = st->entries + capacity;  // the committed slots and this operation's
    if (entries1 >= 0xFFFFFFF0ull) return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 heap entries");
    const uint64_t cand = 2 * entries1;  // every entry is a candidate of its two videos
    if (!(s = st->cur->entry.reserve(entries1, st->entries, stream)).ok() || !(s = st->runs.reserve(capacity)).ok() ||
        !(s = st->scratch.reserve(scratch_buckets, capacity)).ok() || !(s = st->cand.reserve(cand)).ok() ||
        !(s = st->links.reserve(cand)).ok() || !(s = enqueue(capacity, entries1)).ok())
      return s;
    if (out->found <= capacity) {
      out->runs.clear();
      if ((out->failed & kEpilogueBucketTooLarge) && out->found) {
        out->runs.resize(out->found);
        NEEDLE_HIP_TRY(hipMemcpy(out->runs.data(), st->runs.ptr, (size_t)out->found * sizeof(NeedleHipRun), hipMemcpyDeviceToHost));
      }
      return Status::Ok();
    }
    st->capacity = out->found;  // the scan is deterministic: a second pass with the exact size fits
  }
  return Status::Make(NeedleError_Unknown, std::string(what) + ": run list did not fit after resize");
}

// The scan's run list (st->runs, st->run_count) sorted by bucket into the scratch.
Status index_sort_runs(IndexStore *st, uint32_t buckets, uint32_t capacity, hipStream_t stream) {
  RunSegments segs;
  std::memset(&segs, 0, sizeof(segs));
  segs.count = 1;
  segs.found[0] = st->run_count.ptr;
  segs.runs[0] = st->runs.ptr;
  segs.capacity[0] = capacity;
  return enqueue_bucket_sort("index_buckets", segs, buckets, capacity, &st->scratch, stream);
}

// The operation's buckets' entries from the sorted runs, behind the committed entries (part of the store once the append is
// committed or the edit has gathered them), with the row tables `t`.  Inside the caller's timer.
template <class Pairs, class... Extra>
Status index_entries(IndexStore *st, const EpilogueParams &pr, const StoreTables &t, hipStream_t stream, Extra... extra) {
  return enqueue_pair_entries<Pairs, Extra...>(st->device, pr, st->scratch, t.row_len.ptr(), t.row_ts.ptr(), t.row_seek.ptr(), t.ts_table.ptr(),
                                              st->cur->entry.ptr() + st->entries, st->ctl.ptr, stream, extra...);
}

// Inside the caller's "index_best_match" timer, behind the kernels that flag the videos whose candidate list changed: those
// and every video from `from` on listed, and best_match over the list in the tables `t`.
void enqueue_list_and_match(IndexStore *st, const EpilogueParams &pr, uint32_t from, const StoreTables &t, bool grouped, hipStream_t stream) {
  EpilogueControl *ctl = st->ctl.ptr;
  hipLaunchKernelGGL(index_list_kernel, dim3((pr.n + 255) / 256), dim3(256), 0, stream, from, pr.n, st->flag.ptr, &ctl->listed, st->list.ptr);
  if (grouped) {  // the operation's tables: the listed videos' groups
    hipLaunchKernelGGL((best_match_kernel<IndexGroupVideos, IndexGroupView, const uint32_t *, const uint32_t *, const uint64_t *>), dim3(pr.n),
                       dim3(256), 0, stream, pr, t.start.ptr(), t.valid.ptr(), t.entry.ptr(), st->cand.ptr, &ctl->cand_cursor, st->links.ptr,
                       st->results.ptr, &ctl->failed, operation_groups(st), st->list.ptr, &ctl->listed, t.hash_duration.ptr());
    return;
  }
  // one workgroup per video at most; those beyond the list's length return at once
  hipLaunchKernelGGL((best_match_kernel<IndexVideos, const uint32_t *, const uint32_t *, const uint64_t *>), dim3(pr.n), dim3(256), 0, stream, pr,
                     t.start.ptr(), t.valid.ptr(), t.entry.ptr(), st->cand.ptr, &ctl->cand_cursor, st->links.ptr, st->results.ptr, &ctl->failed,
                     st->list.ptr, &ctl->listed, t.hash_duration.ptr());
}

// the runs found, the failure word, the listed videos' results (and `held`, an edit's entry count) into pinned memory; the wait
Status index_copy_out(IndexStore *st, uint32_t n, const uint32_t *held, hipStream_t stream, IndexAppendOut *out) {
  PinnedHead *head = st->pinned;
  uint32_t *list = reinterpret_cast<uint32_t *>(head + 1);
  NeedleHipSearchResult *results = reinterpret_cast<NeedleHipSearchResult *>(list + ((n + 1) & ~1u));
  NEEDLE_HIP_TRY(hipMemcpyAsync(&head->found, st->run_count.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(&head->failed, &st->ctl.ptr->failed, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(&head->listed, &st->ctl.ptr->listed, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  if (held) NEEDLE_HIP_TRY(hipMemcpyAsync(&head->held, held, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(list, st->list.ptr, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(results, st->results.ptr, (size_t)n * sizeof(NeedleHipSearchResult), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  out->found = head->found;
  out->failed = head->failed;
  out->held = held ? head->held : 0;
  const uint32_t listed = std::min(head->listed, n);
  out->videos.assign(list, list + listed);
  out->results.assign(results, results + listed);
  return Status::Ok();
}

// The fallback, both operations': the buckets' entries as the host computed them behind the committed ones, their start /
// valid tables to where the device's would be, the failure word cleared; then `rerun`, the operation's second half (the
// scan's `found` is kept).
template <class Rerun>
Status index_host_entries(IndexStore *st, uint64_t buckets, const std::vector<uint32_t> &start, const std::vector<uint32_t> &valid,
                          const std::vector<IndexEntry> &entries, uint32_t *d_start, uint32_t *d_valid, size_t room, const char *misfit,
                          hipStream_t stream, IndexAppendOut *out, Rerun rerun) {
  if (start.size() != buckets || valid.size() != buckets || st->entries + entries.size() > st->cur->entry.buf.count || buckets > room)
    return Status::Make(NeedleError_InvalidArgument, misfit);
  static_assert(sizeof(IndexEntry) == sizeof(DeviceEntry) && offsetof(IndexEntry, score) == offsetof(DeviceEntry, score) &&
                    offsetof(IndexEntry, dst_hash) == offsetof(DeviceEntry, dst_hash),
                "IndexEntry mirrors DeviceEntry");
  NEEDLE_HIP_TRY(upload(st->cur->entry.ptr() + st->entries, reinterpret_cast<const DeviceEntry *>(entries.data()), entries.size(), stream));
  NEEDLE_HIP_TRY(upload(d_start, start.data(), buckets, stream));
  NEEDLE_HIP_TRY(upload(d_valid, valid.data(), buckets, stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(&st->ctl.ptr->failed, 0, sizeof(uint32_t), stream));
  const uint32_t found = out->found;
  Status s = rerun();
  out->found = found;
  return s;
}

// ---- an append ------------------------------------------------------------------------------------------------------------
// mark the changed videos, list them, best_match over the list; then the copies into pinned memory and a wait for them
Status index_best_and_copy(IndexStore *st, const IndexAppend &a, hipStream_t stream, IndexAppendOut *out) {
  const uint64_t new_buckets = append_buckets(a);
  const EpilogueParams pr = epilogue_params(a, a.large_ok, a.n1, new_buckets);
  NEEDLE_HIP_TRY(hipMemsetAsync(st->flag.ptr, 0, std::max<size_t>(a.n1, 1) * sizeof(uint32_t), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(&st->ctl.ptr->cand_cursor, 0, sizeof(st->ctl.ptr->cand_cursor), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(&st->ctl.ptr->listed, 0, sizeof(uint32_t), stream));
  {
    KernelTimer timer("index_best_match", stream);
    if (new_buckets) {
      const uint32_t grid = (uint32_t)std::min<uint64_t>(4096, (new_buckets + 255) / 256);
      if (a.groups)
        hipLaunchKernelGGL(index_group_changed_kernel, dim3(grid), dim3(256), 0, stream, (uint32_t)new_buckets, a.regions, append_first_pair(a),
                           operation_groups(st), (const uint32_t *)(st->cur->valid.ptr() + st->buckets), st->flag.ptr);
      else
        hipLaunchKernelGGL(index_changed_kernel, dim3(grid), dim3(256), 0, stream, (uint32_t)new_buckets, a.regions, append_first_pair(a),
                           st->cur->valid.ptr() + st->buckets, st->flag.ptr);
    }
    enqueue_list_and_match(st, pr, a.n0, *st->cur, a.groups != nullptr, stream);
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  return index_copy_out(st, a.n1, nullptr, stream, out);
}

}  // namespace

namespace {

// The first half of an append: the new videos' rows, timestamps, hash durations and hashes go in behind the committed ones.
Status index_append_tables(IndexStore *st, const IndexAppend &a, hipStream_t stream) {
  if (a.n0 != st->n || a.n1 <= a.n0 || a.regions < 1 || a.regions > 2)
    return Status::Make(NeedleError_InvalidArgument, "index append: inconsistent sizes");
  if (a.groups && (a.groups->group_of.size() != a.n1 || a.groups->vbase[a.n0] * a.regions != st->buckets))
    return Status::Make(NeedleError_InvalidArgument, "index append: the group tables are not the store's list and the new videos");
  StoreTables &t = *st->cur;
  const uint64_t new_buckets = append_buckets(a), buckets1 = st->buckets + new_buckets;
  const uint64_t rows1 = st->rows + a.num_rows, ts1 = st->ts + a.num_ts, hashes1 = st->hashes + a.num_hashes;
  if (buckets1 >= 0xFFFFFFF0ull || hashes1 > UINT32_MAX)
    return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 hashes or sequence pairs");
  Status s;
  if (!(s = t.hash.reserve(std::max<uint64_t>(hashes1, 1), st->hashes, stream)).ok() || !(s = t.row_len.reserve(rows1, st->rows, stream)).ok() ||
      !(s = t.row_ts.reserve(rows1, st->rows, stream)).ok() || !(s = t.row_seek.reserve(rows1, st->rows, stream)).ok() ||
      !(s = t.ts_table.reserve(std::max<uint64_t>(ts1, 1), st->ts, stream)).ok() || !(s = t.hash_duration.reserve(a.n1, st->n, stream)).ok() ||
      !(s = t.start.reserve(std::max<uint64_t>(buckets1, 1), st->buckets, stream)).ok() ||
      !(s = t.valid.reserve(std::max<uint64_t>(buckets1, 1), st->buckets, stream)).ok())
    return s;
  NEEDLE_HIP_TRY(upload(t.hash.ptr() + st->hashes, a.hashes, a.num_hashes, stream));
  NEEDLE_HIP_TRY(upload(t.row_len.ptr() + st->rows, a.row_len, a.num_rows, stream));
  NEEDLE_HIP_TRY(upload(t.row_ts.ptr() + st->rows, a.row_ts, a.num_rows, stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(t.row_seek.ptr() + st->rows, 0, a.num_rows * sizeof(uint64_t), stream));
  NEEDLE_HIP_TRY(upload(t.ts_table.ptr() + st->ts, a.ts, a.num_ts, stream));
  NEEDLE_HIP_TRY(upload(t.hash_duration.ptr() + st->n, a.hash_duration, a.n1 - a.n0, stream));
  return a.groups ? index_upload_groups(st, *a.groups, stream) : Status::Ok();
}

// The second half, behind the slab: fill(capacity) leaves the new pairs' runs, tagged for the append, in st->runs and their
// number in st->run_count (the scan, or a matcher's list ingested); then the entries into the store, best_match over the
// changed videos and the copies.
template <class Fill>
Status index_append_from_slab(IndexStore *st, const IndexAppend &a, hipStream_t stream, IndexAppendOut *out, Fill fill) {
  StoreTables &t = *st->cur;
  const uint64_t new_buckets = append_buckets(a);
  return index_run(st, "index append", a.num_problems, new_buckets, a.n1, stream, out, [&](uint32_t capacity, uint64_t) -> Status {
    Status s = fill(capacity);
    if (!s.ok()) return s;
    NEEDLE_HIP_TRY(hipMemsetAsync(st->ctl.ptr, 0, sizeof(EpilogueControl), stream));
    if (new_buckets) {
      const EpilogueParams pr = epilogue_params(a, a.large_ok, a.n1, new_buckets);
      if (!(s = index_sort_runs(st, pr.buckets, capacity, stream)).ok()) return s;
      {
        KernelTimer timer("index_entries", stream);
        s = a.groups ? index_entries<IndexGroupAppendPairs, IndexGroupView, uint64_t>(st, pr, t, stream, operation_groups(st), append_first_pair(a))
                     : index_entries<ColumnMajorPairs, uint64_t>(st, pr, t, stream, append_first_pair(a));
        if (!s.ok()) return s;
        // into the store's tables: start = where the entries were written
        hipLaunchKernelGGL(index_store_buckets_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (new_buckets + 255) / 256)), dim3(256), 0,
                           stream, pr.buckets, st->scratch.start.ptr, st->scratch.valid.ptr, (uint32_t)st->entries, t.start.ptr() + st->buckets,
                           t.valid.ptr() + st->buckets);
      }
      NEEDLE_HIP_TRY(hipGetLastError());
    }
    return index_best_and_copy(st, a, stream, out);
  });
}

}  // namespace

Status gpu_index_append(IndexStore *st, const IndexAppend &a, IndexAppendOut *out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = index_enter(st);
  if (!s.ok()) return s;
  hipStream_t stream = library_stream();
  if (!(s = index_append_tables(st, a, stream)).ok()) return s;
  return index_append_from_slab(st, a, stream, out, [&](uint32_t capacity) -> Status {
    // the scan of the new pairs only (every form eligible), behind the uploads on the same stream
    return gpu_hamming_runs_device(st->cur->hash.ptr(), a.seqs, a.num_seqs, a.problems, a.num_problems, a.threshold, st->runs.ptr, capacity,
                                   st->run_count.ptr, false, false);
  });
}

namespace {

// An append whose slab is filled from run lists that were uploaded, not by the scan: `runs` and every row's min_len go up,
// launch(capacity) enqueues the kernels that compare the rows and ingest the list, and the error word comes back in
// out->refused once everything behind them has run.
template <class Launch>
Status index_append_ingested(IndexStore *st, const IndexAppend &a, const NeedleHipRun *runs, size_t num_runs, const uint32_t *min_len,
                             hipStream_t stream, IndexAppendOut *out, Launch launch) {
  const size_t rows = (size_t)a.n1 * a.regions;
  Status s;
  if (!(s = st->matched_runs.reserve(std::max<size_t>(num_runs, 1))).ok() || !(s = st->matched_min_len.reserve(rows)).ok() ||
      !(s = st->matched_error.reserve(1)).ok())
    return s;
  NEEDLE_HIP_TRY(upload(st->matched_runs.ptr, runs, num_runs, stream));
  NEEDLE_HIP_TRY(upload(st->matched_min_len.ptr, min_len, rows, stream));
  const uint32_t capacity_before = st->capacity;
  st->capacity = std::max<uint32_t>(st->capacity, (uint32_t)num_runs);  // the survivors are at most the list: one pass
  s = index_append_from_slab(st, a, stream, out, [&](uint32_t capacity) -> Status {
    NEEDLE_HIP_TRY(hipMemsetAsync(st->matched_error.ptr, 0, sizeof(uint32_t), stream));
    NEEDLE_HIP_TRY(hipMemsetAsync(st->run_count.ptr, 0, sizeof(uint32_t), stream));
    KernelTimer timer("index_ingest", stream);
    launch(capacity);
    NEEDLE_HIP_TRY(hipGetLastError());
    return Status::Ok();
  });
  if (s.ok()) {
    const hipError_t e = hipMemcpy(&out->refused, st->matched_error.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) s = Status::Make(NeedleError_Unknown, std::string("HIP error: ") + hipGetErrorString(e) + " reading the ingest's error word");
  }
  if (!s.ok() || out->refused) st->capacity = capacity_before;  // a call that commits nothing sizes nothing for the next one
  return s;
}

}  // namespace

Status gpu_index_append_matched(IndexStore *st, const IndexAppend &a, const IndexMatched &m, IndexAppendOut *out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = index_enter(st);
  if (!s.ok()) return s;
  hipStream_t stream = library_stream();
  if (m.num_runs > 0x7fffffffu) return Status::Make(NeedleError_InvalidArgument, "index add_matched: more than 2^31 runs");
  if (!(s = index_append_tables(st, a, stream)).ok()) return s;
  if (!(s = st->segments.reserve(std::max<size_t>(m.num_lanes, 1))).ok()) return s;
  NEEDLE_HIP_TRY(upload(st->segments.ptr, m.lanes, m.num_lanes, stream));
  GroupView from{};  // a grouped index: the matcher's numbering over the operation's list, its tables the ones just uploaded
  if (a.groups) {
    if (!(s = st->matched_base.reserve(a.groups->base.size())).ok()) return s;
    NEEDLE_HIP_TRY(upload(st->matched_base.ptr, a.groups->base.data(), a.groups->base.size(), stream));
    const IndexGroupView &to = operation_groups(st);
    from = GroupView{to.group_of, to.rank_of, to.size, to.first, st->matched_base.ptr, to.members, (uint32_t)a.groups->size.size()};
  }
  return index_append_ingested(st, a, m.runs, m.num_runs, m.min_len, stream, out, [&](uint32_t capacity) {
    if (m.num_lanes)
      hipLaunchKernelGGL(index_compare_rows_kernel, dim3((uint32_t)std::min<size_t>(m.num_lanes, 4096)), dim3(256), 0, stream,
                         (const IndexSegment *)st->segments.ptr, (uint32_t)m.num_lanes, (const uint32_t *)st->cur->hash.ptr(), m.history,
                         st->matched_error.ptr);
    if (m.num_runs && a.groups)
      hipLaunchKernelGGL(index_ingest_runs_grouped_kernel, dim3((uint32_t)std::min<size_t>(4096, (m.num_runs + 255) / 256)), dim3(256), 0, stream,
                         (const NeedleHipRun *)st->matched_runs.ptr, (uint32_t)m.num_runs, from, operation_groups(st), append_first_pair(a), a.n0,
                         a.regions, (const uint32_t *)st->matched_min_len.ptr, (const uint32_t *)st->cur->row_len.ptr(), st->runs.ptr, capacity,
                         st->run_count.ptr, st->matched_error.ptr);
    else if (m.num_runs)
      hipLaunchKernelGGL(index_ingest_runs_kernel, dim3((uint32_t)std::min<size_t>(4096, (m.num_runs + 255) / 256)), dim3(256), 0, stream,
                         (const NeedleHipRun *)st->matched_runs.ptr, (uint32_t)m.num_runs, a.n1, a.n0, a.regions,
                         (const uint32_t *)st->matched_min_len.ptr, (const uint32_t *)st->cur->row_len.ptr(), st->runs.ptr, capacity,
                         st->run_count.ptr, st->matched_error.ptr);
  });
}

Status gpu_index_append_streamed(IndexStore *st, const IndexAppend &a, const IndexStreamed &m, IndexAppendOut *out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = index_enter(st);
  if (!s.ok()) return s;
  hipStream_t stream = library_stream();
  const size_t num_runs = m.num_matcher_runs + m.num_cross_runs;
  if (num_runs > 0x7fffffffu) return Status::Make(NeedleError_InvalidArgument, "index add_streamed: more than 2^31 runs");
  if (!(s = index_append_tables(st, a, stream)).ok()) return s;
  if (!(s = st->lane_rows.reserve(std::max<size_t>(m.num_lanes, 1))).ok() || !(s = st->run_lane.reserve(std::max<size_t>(m.num_matcher_runs, 1))).ok())
    return s;
  NEEDLE_HIP_TRY(upload(st->lane_rows.ptr, m.lanes, m.num_lanes, stream));
  NEEDLE_HIP_TRY(upload(st->run_lane.ptr, m.run_lane, m.num_matcher_runs, stream));
  return index_append_ingested(st, a, m.runs, num_runs, m.min_len, stream, out, [&](uint32_t capacity) {
    if (m.num_lanes)
      hipLaunchKernelGGL(index_compare_lanes_kernel, dim3((uint32_t)std::min<size_t>(m.num_lanes, 4096)), dim3(256), 0, stream,
                         (const IndexLaneRow *)st->lane_rows.ptr, (uint32_t)m.num_lanes, (const uint32_t *)st->cur->hash.ptr(),
                         st->matched_error.ptr);
    if (num_runs)
      hipLaunchKernelGGL(index_ingest_streamed_kernel, dim3((uint32_t)std::min<size_t>(4096, (num_runs + 255) / 256)), dim3(256), 0, stream,
                         (const NeedleHipRun *)st->matched_runs.ptr, (uint32_t)m.num_matcher_runs, (uint32_t)num_runs,
                         (const uint32_t *)st->run_lane.ptr, a.n0, a.n1, a.regions, (const uint32_t *)st->matched_min_len.ptr,
                         (const uint32_t *)st->cur->row_len.ptr(), st->runs.ptr, capacity, st->run_count.ptr, st->matched_error.ptr);
  });
}

Status gpu_index_append_host_entries(IndexStore *st, const IndexAppend &a, const std::vector<uint32_t> &start,
                                     const std::vector<uint32_t> &valid, const std::vector<IndexEntry> &entries, IndexAppendOut *out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  hipStream_t stream = library_stream();
  std::vector<uint32_t> shifted(start);  // relative to the append's first entry -> the store's slots
  for (uint32_t &x : shifted) x += (uint32_t)st->entries;
  return index_host_entries(st, append_buckets(a), shifted, valid, entries, st->cur->start.ptr() + st->buckets, st->cur->valid.ptr() + st->buckets,
                            st->cur->valid.buf.count - st->buckets, "index append: host entries do not fit the append", stream, out,
                            [&] { return index_best_and_copy(st, a, stream, out); });
}

void index_store_commit(IndexStore *st, const IndexAppend &a, uint32_t found) {
  st->buckets += append_buckets(a);
  st->entries += found;
  st->rows += a.num_rows;
  st->ts += a.num_ts;
  st->hashes += a.num_hashes;
  st->n = a.n1;
  if (a.groups) st->group_cur = 1 - st->group_cur;
}

// ---- an edit: removal / replacement --------------------------------------------------------------------------------------
namespace {

// The first half of an edit: the maps and the new rows' tables uploaded, the kept rows gathered into the second arena and
// timestamp table, the fresh rows behind them; the scan of the listed pairs and their entries behind the committed ones.
Status index_edit_tables(IndexStore *st, const IndexEdit &e, uint32_t capacity, hipStream_t stream) {
  const StoreTables &cur = *st->cur, &next = *st->next;
  const uint32_t R = e.regions;
  const uint64_t rows = (uint64_t)e.n_new * R, listed = (uint64_t)e.num_pairs * R;
  NEEDLE_HIP_TRY(upload(st->old_of_new.ptr, e.old_of_new, e.n_new, stream));
  NEEDLE_HIP_TRY(upload(st->new_of_old.ptr, e.new_of_old, e.n_old, stream));
  NEEDLE_HIP_TRY(upload(st->gone.ptr, e.gone, e.num_gone, stream));
  NEEDLE_HIP_TRY(upload(st->pair_ids.ptr, e.pair_ids, e.num_pairs, stream));
  NEEDLE_HIP_TRY(upload(st->segments.ptr, e.hash_rows, e.num_hash_rows, stream));
  NEEDLE_HIP_TRY(upload(st->segments.ptr + e.num_hash_rows, e.ts_rows, e.num_ts_rows, stream));
  NEEDLE_HIP_TRY(upload(next.hash.ptr() + (e.total_hashes - e.num_hashes), e.hashes, e.num_hashes, stream));
  NEEDLE_HIP_TRY(upload(next.ts_table.ptr() + (e.total_ts - e.num_ts), e.ts, e.num_ts, stream));
  NEEDLE_HIP_TRY(upload(next.row_len.ptr(), e.row_len, rows, stream));
  NEEDLE_HIP_TRY(upload(next.row_ts.ptr(), e.row_ts, rows, stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(next.row_seek.ptr(), 0, rows * sizeof(uint64_t), stream));
  NEEDLE_HIP_TRY(upload(next.hash_duration.ptr(), e.hash_duration, e.n_new, stream));
  {
    KernelTimer timer("index_copy_rows", stream);
    if (e.num_hash_rows)
      hipLaunchKernelGGL(index_copy_rows_kernel<uint32_t>, dim3((uint32_t)std::min<size_t>(e.num_hash_rows, 4096)), dim3(256), 0, stream,
                         (const IndexSegment *)st->segments.ptr, (uint32_t)e.num_hash_rows, (const uint32_t *)cur.hash.ptr(), next.hash.ptr());
    if (e.num_ts_rows)
      hipLaunchKernelGGL(index_copy_rows_kernel<uint64_t>, dim3((uint32_t)std::min<size_t>(e.num_ts_rows, 4096)), dim3(256), 0, stream,
                         (const IndexSegment *)(st->segments.ptr + e.num_hash_rows), (uint32_t)e.num_ts_rows,
                         (const uint64_t *)cur.ts_table.ptr(), next.ts_table.ptr());
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  NEEDLE_HIP_TRY(hipMemsetAsync(st->ctl.ptr, 0, sizeof(EpilogueControl), stream));
  if (!e.num_problems) {
    NEEDLE_HIP_TRY(hipMemsetAsync(st->run_count.ptr, 0, sizeof(uint32_t), stream));
  } else {
    Status s = gpu_hamming_runs_device(next.hash.ptr(), e.seqs, rows, e.problems, e.num_problems, e.threshold, st->runs.ptr, capacity,
                                       st->run_count.ptr, false, false);
    if (!s.ok()) return s;
  }
  if (!listed) return Status::Ok();
  const EpilogueParams pr = epilogue_params(e, e.large_ok, e.n_new, listed);
  NEEDLE_HIP_TRY(hipMemsetAsync(st->scratch.valid.ptr, 0, listed * sizeof(uint32_t), stream));  // (a bucket the device does not order: 0)
  Status s = index_sort_runs(st, pr.buckets, capacity, stream);
  if (!s.ok()) return s;
  {
    KernelTimer timer("index_entries", stream);
    s = e.groups ? index_entries<IndexGroupListedPairs, IndexGroupView, const uint32_t *>(st, pr, next, stream, operation_groups(st), st->pair_ids.ptr)
                 : index_entries<ListedPairs, const uint32_t *>(st, pr, next, stream, st->pair_ids.ptr);
    if (!s.ok()) return s;
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

// The second half: every bucket's count and source (kept pairs from the committed store, listed ones from this edit's
// entries), their starts, the gather into the second entry buffer, the videos to recompute and their best match over the
// rebuilt store; the copies and the wait.
Status index_edit_rebuild(IndexStore *st, const IndexEdit &e, hipStream_t stream, IndexAppendOut *out) {
  const StoreTables &cur = *st->cur, &next = *st->next;
  const uint32_t R = e.regions, n = e.n_new;
  const uint64_t buckets = edit_buckets(e), listed = (uint64_t)e.num_pairs * R;
  {
    KernelTimer timer("index_rebuild", stream);
    if (buckets) {
      if (e.groups)
        hipLaunchKernelGGL(index_group_edit_buckets_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (buckets + 255) / 256)), dim3(256), 0, stream,
                           (uint32_t)buckets, R, operation_groups(st), committed_groups(st), (const uint32_t *)st->old_of_new.ptr,
                           (const uint32_t *)cur.start.ptr(), (const uint32_t *)cur.valid.ptr(), st->src.ptr, next.valid.ptr());
      else
        hipLaunchKernelGGL(index_edit_buckets_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (buckets + 255) / 256)), dim3(256), 0, stream,
                           (uint32_t)buckets, R, (const uint32_t *)st->old_of_new.ptr, (const uint32_t *)cur.start.ptr(),
                           (const uint32_t *)cur.valid.ptr(), st->src.ptr, next.valid.ptr());
      if (listed)
        hipLaunchKernelGGL(index_edit_fresh_kernel, dim3((uint32_t)std::min<uint64_t>(4096, (listed + 255) / 256)), dim3(256), 0, stream,
                           (uint32_t)listed, R, (const uint32_t *)st->pair_ids.ptr, (const uint32_t *)st->scratch.start.ptr,
                           (const uint32_t *)st->scratch.valid.ptr, (uint32_t)st->entries, st->src.ptr, next.valid.ptr());
      enqueue_exclusive_scan(next.valid.ptr(), (uint32_t)buckets, st->scratch.sums.ptr, next.start.ptr(), stream);
    } else {
      NEEDLE_HIP_TRY(hipMemsetAsync(next.start.ptr(), 0, sizeof(uint32_t), stream));
    }
  }
  if (buckets) {
    KernelTimer timer("index_gather", stream);
    const uint64_t max_entries = next.entry.buf.count;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(8192, (3 * max_entries + 255) / 256);
    hipLaunchKernelGGL(index_gather_kernel, dim3(std::max(grid, 1u)), dim3(256), 0, stream, (uint32_t)buckets, (const uint32_t *)next.start.ptr(),
                       (const uint32_t *)st->src.ptr, reinterpret_cast<const uint4 *>(cur.entry.ptr()),
                       reinterpret_cast<uint4 *>(next.entry.ptr()), max_entries);
  }
  const EpilogueParams pr = epilogue_params(e, e.large_ok, n, buckets);
  NEEDLE_HIP_TRY(hipMemsetAsync(&st->ctl.ptr->cand_cursor, 0, sizeof(st->ctl.ptr->cand_cursor), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(&st->ctl.ptr->listed, 0, sizeof(uint32_t), stream));
  {
    KernelTimer timer("index_best_match", stream);
    hipLaunchKernelGGL(index_fresh_flags_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, (const uint32_t *)st->old_of_new.ptr, st->flag.ptr);
    if (e.num_gone && e.n_old > 1) {
      const uint64_t work = (uint64_t)e.num_gone * e.n_old;
      const dim3 grid((uint32_t)std::min<uint64_t>(4096, (work + 255) / 256));
      if (e.groups)
        hipLaunchKernelGGL(index_group_gone_partners_kernel, grid, dim3(256), 0, stream, e.n_old, R, committed_groups(st),
                           (const uint32_t *)st->gone.ptr, (uint32_t)e.num_gone, (const uint32_t *)cur.valid.ptr(),
                           (const uint32_t *)st->new_of_old.ptr, st->flag.ptr);
      else
        hipLaunchKernelGGL(index_gone_partners_kernel, grid, dim3(256), 0, stream, e.n_old, R, (const uint32_t *)st->gone.ptr,
                           (uint32_t)e.num_gone, (const uint32_t *)cur.valid.ptr(), (const uint32_t *)st->new_of_old.ptr, st->flag.ptr);
    }
    if (listed) {
      const dim3 grid((uint32_t)std::min<uint64_t>(4096, (listed + 255) / 256));
      if (e.groups)
        hipLaunchKernelGGL(index_group_fresh_partners_kernel, grid, dim3(256), 0, stream, (uint32_t)listed, R, operation_groups(st),
                           (const uint32_t *)st->pair_ids.ptr, (const uint32_t *)st->scratch.valid.ptr, st->flag.ptr);
      else
        hipLaunchKernelGGL(index_fresh_partners_kernel, grid, dim3(256), 0, stream, (uint32_t)listed, R, (const uint32_t *)st->pair_ids.ptr,
                           (const uint32_t *)st->scratch.valid.ptr, st->flag.ptr);
    }
    enqueue_list_and_match(st, pr, n, next, e.groups != nullptr, stream);
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  return index_copy_out(st, n, next.start.ptr() + buckets, stream, out);
}

}  // namespace

Status gpu_index_edit(IndexStore *st, const IndexEdit &e, IndexAppendOut *out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = index_enter(st);
  if (!s.ok()) return s;
  if (e.n_old != st->n || e.n_new < 1 || e.regions < 1 || e.regions > 2)
    return Status::Make(NeedleError_InvalidArgument, "index edit: inconsistent sizes");
  if (e.groups && (e.groups->group_of.size() != e.n_new || committed_groups(st).videos != e.n_old))
    return Status::Make(NeedleError_InvalidArgument, "index edit: the group tables are not the new list's, or the store is not a grouped one");
  hipStream_t stream = library_stream();
  if (e.groups && !(s = index_upload_groups(st, *e.groups, stream)).ok()) return s;
  StoreTables &next = *st->next;
  const uint64_t buckets = edit_buckets(e), listed = (uint64_t)e.num_pairs * e.regions, rows = (uint64_t)e.n_new * e.regions;
  if (buckets >= 0xFFFFFFF0ull || e.total_hashes > UINT32_MAX || e.total_ts > UINT32_MAX)
    return Status::Make(NeedleError_InvalidArgument, "index too large: more than 2^32 hashes or sequence pairs");
  if (!(s = next.hash.reserve(std::max<uint64_t>(e.total_hashes, 1), 0, stream)).ok() ||
      !(s = next.ts_table.reserve(std::max<uint64_t>(e.total_ts, 1), 0, stream)).ok() || !(s = next.row_len.reserve(rows, 0, stream)).ok() ||
      !(s = next.row_ts.reserve(rows, 0, stream)).ok() || !(s = next.row_seek.reserve(rows, 0, stream)).ok() ||
      !(s = next.hash_duration.reserve(e.n_new, 0, stream)).ok() || !(s = next.start.reserve(buckets + 1, 0, stream)).ok() ||
      !(s = next.valid.reserve(std::max<uint64_t>(buckets, 1), 0, stream)).ok() || !(s = st->src.reserve(std::max<uint64_t>(buckets, 1))).ok() ||
      !(s = st->old_of_new.reserve(e.n_new)).ok() || !(s = st->new_of_old.reserve(std::max<uint32_t>(e.n_old, 1))).ok() ||
      !(s = st->gone.reserve(std::max<size_t>(e.num_gone, 1))).ok() || !(s = st->pair_ids.reserve(std::max<size_t>(e.num_pairs, 1))).ok() ||
      !(s = st->segments.reserve(std::max<size_t>(e.num_hash_rows + e.num_ts_rows, 1))).ok() ||
      !(s = st->scratch.sums.reserve(EntriesScratch::sums_for(buckets))).ok())  // (the rebuilt store's scan; the listed buckets' is index_run's)
    return s;
  // the rebuilt store holds at most the committed slots and this edit's
  return index_run(st, "index edit", e.num_problems, listed, e.n_new, stream, out, [&](uint32_t capacity, uint64_t entries1) -> Status {
    Status s = next.entry.reserve(entries1, 0, stream);
    if (!s.ok() || !(s = index_edit_tables(st, e, capacity, stream)).ok()) return s;
    return index_edit_rebuild(st, e, stream, out);
  });
}

Status gpu_index_edit_host_entries(IndexStore *st, const IndexEdit &e, const std::vector<uint32_t> &start, const std::vector<uint32_t> &valid,
                                   const std::vector<IndexEntry> &entries, IndexAppendOut *out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  hipStream_t stream = library_stream();
  return index_host_entries(st, (uint64_t)e.num_pairs * e.regions, start, valid, entries, st->scratch.start.ptr, st->scratch.valid.ptr,
                            st->scratch.valid.count, "index edit: host entries do not fit the edit", stream, out,
                            [&] { return index_edit_rebuild(st, e, stream, out); });
}

void index_store_switch(IndexStore *st, const IndexEdit &e, uint32_t held) {
  std::swap(st->cur, st->next);
  st->n = e.n_new;
  st->buckets = edit_buckets(e);
  st->entries = held;
  st->rows = (uint64_t)e.n_new * e.regions;
  st->ts = e.total_ts;
  st->hashes = e.total_hashes;
  if (e.groups) st->group_cur = 1 - st->group_cur;
}

void index_store_clear(IndexStore *st) {
  st->n = 0;
  st->buckets = st->entries = st->rows = st->ts = st->hashes = 0;
  st->group_tables[st->group_cur].view = IndexGroupView{};  // (a grouped index: no video, no table is read)
}

// ---- match evidence -------------------------------------------------------------------------------------------------------
// best_match over every committed video under EvidenceVideos (the selection itself, with the winners' index, links and score
// written out), then match_evidence_kernel over the same videos, which reads those and the candidate pool the first launch
// filled.  The committed tables are only read; the candidate pool, the links, the results slots and the control words are an
// operation's scratch, which every operation sets up again before it reads it.
Status gpu_index_evidence(IndexStore *st, const IndexOptions &o, NeedleHipSearchEvidence *evidence) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = ensure_device();
  if (!s.ok() || !(s = index_check_device(st)).ok()) return s;
  const uint32_t n = st->n;
  if (!n) return Status::Ok();
  hipStream_t stream = library_stream();
  const uint64_t cand = std::max<uint64_t>(2 * st->entries, 1);  // every entry is a candidate of its two videos
  if (!(s = st->ctl.reserve(1)).ok() || !(s = st->results.reserve(n)).ok() || !(s = st->cand.reserve(cand)).ok() ||
      !(s = st->links.reserve(cand)).ok() || !(s = st->winners.reserve(n)).ok() || !(s = st->evidence.reserve(n)).ok())
    return s;
  if (n > st->evidence_pinned_count) {
    if (st->evidence_pinned) (void)hipHostFree(st->evidence_pinned);
    st->evidence_pinned = nullptr;
    st->evidence_pinned_count = 0;
    NEEDLE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&st->evidence_pinned), 2 * (size_t)n * sizeof(NeedleHipSearchEvidence), hipHostMallocDefault));
    st->evidence_pinned_count = 2 * (size_t)n;
  }
  const StoreTables &t = *st->cur;
  const EpilogueParams pr = epilogue_params(o, o.large_ok, n, st->buckets);
  EpilogueControl *ctl = st->ctl.ptr;
  NEEDLE_HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(EpilogueControl), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(st->winners.ptr, 0, (size_t)n * sizeof(DeviceWinners), stream));
  const IndexGroupView groups = o.groups ? committed_groups(st) : IndexGroupView{};  // a grouped index: both launches under the committed tables
  if (o.groups && groups.videos != n) return Status::Make(NeedleError_InvalidArgument, "index evidence: the store holds no group tables for its videos");
  {
    KernelTimer timer("index_evidence_match", stream);
    if (o.groups)
      hipLaunchKernelGGL((best_match_kernel<IndexGroupEvidenceVideos, IndexGroupView, const uint64_t *, DeviceWinners *>), dim3(n), dim3(256), 0,
                         stream, pr, t.start.ptr(), t.valid.ptr(), t.entry.ptr(), st->cand.ptr, &ctl->cand_cursor, st->links.ptr, st->results.ptr,
                         &ctl->failed, groups, t.hash_duration.ptr(), st->winners.ptr);
    else
      hipLaunchKernelGGL((best_match_kernel<EvidenceVideos, const uint64_t *, DeviceWinners *>), dim3(n), dim3(256), 0, stream, pr, t.start.ptr(),
                         t.valid.ptr(), t.entry.ptr(), st->cand.ptr, &ctl->cand_cursor, st->links.ptr, st->results.ptr, &ctl->failed,
                         t.hash_duration.ptr(), st->winners.ptr);
  }
  {
    KernelTimer timer("index_evidence", stream);
    if (o.groups)
      hipLaunchKernelGGL((match_evidence_kernel<IndexGroupEvidenceVideos, IndexGroupView, const uint64_t *, DeviceWinners *>), dim3(n), dim3(256), 0,
                         stream, pr, (const uint32_t *)t.start.ptr(), (const uint32_t *)t.valid.ptr(), (const DeviceEntry *)t.entry.ptr(),
                         (const Candidate *)st->cand.ptr, st->evidence.ptr, groups, (const uint64_t *)t.hash_duration.ptr(), st->winners.ptr);
    else
      hipLaunchKernelGGL((match_evidence_kernel<EvidenceVideos, const uint64_t *, DeviceWinners *>), dim3(n), dim3(256), 0, stream, pr,
                         (const uint32_t *)t.start.ptr(), (const uint32_t *)t.valid.ptr(), (const DeviceEntry *)t.entry.ptr(),
                         (const Candidate *)st->cand.ptr, st->evidence.ptr, (const uint64_t *)t.hash_duration.ptr(), st->winners.ptr);
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  NEEDLE_HIP_TRY(hipMemcpyAsync(st->evidence_pinned, st->evidence.ptr, (size_t)n * sizeof(NeedleHipSearchEvidence), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  std::memcpy(evidence, st->evidence_pinned, (size_t)n * sizeof(NeedleHipSearchEvidence));
  return Status::Ok();
}

int index_store_device(const IndexStore *st) { return st->device; }

Status index_store_arena(IndexStore *st, const uint32_t **d_hashes) {
  *d_hashes = nullptr;
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = ensure_device();
  if (!s.ok() || !(s = index_check_device(st)).ok()) return s;
  if (st->hashes) *d_hashes = st->cur->hash.ptr();
  return Status::Ok();
}

Status index_store_sizes(IndexStore *st, uint64_t sizes[4]) {
  sizes[0] = 0;
  sizes[1] = st->entries;
  sizes[2] = st->hashes;
  sizes[3] = st->ts;
  if (!st->buckets) return Status::Ok();
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = index_check_device(st);
  if (!s.ok()) return s;
  std::vector<uint32_t> valid(st->buckets);
  hipStream_t stream = library_stream();
  NEEDLE_HIP_TRY(hipMemcpyAsync(valid.data(), st->cur->valid.ptr(), valid.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  for (uint32_t v : valid) sizes[0] += v;
  return Status::Ok();
}

}  // namespace needle
