// Device form of the per-video epilogue of a library job (epilogue.hip); the host form is comparator.cpp.
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdint>
#include <vector>

#include "../../include/needle_hip.h"
#include "common.h"

namespace needle {

struct EpilogueJob {
  int slot = 0;                      // job slot: two jobs in flight keep two workspaces
  uint32_t n = 0;                    // videos
  uint32_t regions = 1;              // of the COMPARATOR: NeedleHipRun.problem = pair * regions + region
  uint32_t rows_per_video = 1;       // of the library's hash arena: row = video * rows_per_video + region
  uint32_t v0 = 0, v1 = 0;           // results wanted for videos [v0, v1)
  uint32_t threshold = 0;
  bool include_endings = false;
  ns_t min_opening_duration = 0, min_ending_duration = 0, time_padding = 0, hash_duration = 0;
  // the run list: num_segments pieces in order (a rank's slab, the gathered heads in rank order, or the buffer of a
  // host-side search call), each a device word holding the runs found and up to segment_capacity runs
  const uint32_t *segment_count[64] = {nullptr};
  const NeedleHipRun *segment_runs[64] = {nullptr};
  int num_segments = 0;
  uint32_t segment_capacity = 0;
  uint32_t segment_capacities[64] = {0};  // per segment where they differ (the owner-directed exchange's blocks); 0 = segment_capacity
  uint64_t max_runs = 0;             // upper bound of the runs in all segments (sizes the workspaces)
  // per arena row: hashes kept, offset of its (un-seeked) timestamps in `ts`, seek added to each of them
  const std::vector<uint32_t> *row_len = nullptr, *row_ts = nullptr;
  const std::vector<uint64_t> *row_seek = nullptr, *ts = nullptr;
};

// The device form gives a pair's runs to ONE lane (insertion order + heap): a pair with more runs than this (silence against
// silence, one sustained tone against itself) would keep that lane busy for seconds; such a bucket is a workgroup's (below).
// Bit 31 of the failure word: the caller computes the results with the host form (threaded, n log n) from the run list.
// NEEDLE_HIP_EPILOGUE_BUCKET_LIMIT is not a switch: tests lower the constant by building with -D.
#ifndef NEEDLE_EPILOGUE_BUCKET_LIMIT
#define NEEDLE_EPILOGUE_BUCKET_LIMIT 24
#endif
constexpr uint32_t kEpilogueBucketLimit = NEEDLE_EPILOGUE_BUCKET_LIMIT;
// Round 6: buckets beyond that limit (up to kEpilogueLargeLimit runs: two fully silent 24-minute windows are 5 800) go to a
// WORKGROUP each (pair_entries_large_kernel: bitonic sort into the walk order and the heap's sift-ups on packed 64-bit keys in
// LDS) instead of failing the job over to the host.  Only a bucket beyond kEpilogueLargeLimit, a row of 65 536 hashes or more, or
// timestamps that do not strictly increase (the packed key stands for them) still set the bit.
#ifndef NEEDLE_EPILOGUE_LARGE_LIMIT
#define NEEDLE_EPILOGUE_LARGE_LIMIT 8192
#endif
constexpr uint32_t kEpilogueLargeLimit = NEEDLE_EPILOGUE_LARGE_LIMIT;
constexpr uint32_t kEpilogueBucketTooLarge = 0x80000000u;
// Jobs whose device epilogue was handed back to the host because of that bit (needle_hip_epilogue_host_fallbacks): a
// silent performance cliff otherwise -- one pair of silent stretches moves a whole library's epilogue to the host.
std::atomic<uint64_t> &epilogue_host_fallbacks();
// (host side of both callers: counts, and says so under NEEDLE_HIP_TRACE)
void note_epilogue_host_fallback(const char *where, size_t runs, size_t videos);

// The owner-directed exchange's send side (round 6, library.cpp): the runs of a rank's slab sorted into one block per
// destination rank -- a run of pair (i, j) goes to the owners of video i and of video j (videos in blocks of `videos_per_rank`:
// the sharded epilogue's blocks, comparator.rs:583-588 needs a video's pairs and nothing else).  A block = a slab: 32-byte
// header (word 0: runs DIRECTED to it, which may exceed what it holds -- the caller's overflow test) + capacity[q] runs, at
// send + offset[q] bytes.  Enqueued on `stream`; the headers are cleared first.
struct DirectPlan {
  uint32_t offset[64];    // bytes
  uint32_t capacity[64];  // runs
};
Status gpu_direct_runs(const uint32_t *d_found, const NeedleHipRun *d_runs, uint32_t slab_capacity, uint32_t n, uint32_t regions,
                       uint32_t videos_per_rank, int world, uint8_t *d_send, const DirectPlan &plan, hipStream_t stream);

// Enqueues the epilogue kernels on `stream` behind whatever fills the segments, then the copies of results[n] and of the
// failure count (videos whose padding / hash duration exceed the match end: the reference panics) into HOST memory
// (pinned: the copies are asynchronous).  Counts beyond a segment's capacity are clamped: the host redoes such a job.
Status gpu_epilogue_enqueue(const EpilogueJob &job, hipStream_t stream, NeedleHipSearchResult *host_results, uint32_t *host_failed);

// Comparator::run_with_frame_hashes with both halves on the device (search.hip): host hash arena in, scan + simhash, the
// epilogue above on the run list where it lies, the n per-video results out; the run list itself never crosses PCIe.
// `job` carries everything but the segments.  *failed != 0 (a failing video, or kEpilogueBucketTooLarge): the caller falls
// back to the host epilogue (which reports the video that fails, in the reference's order) -- `runs` then holds the
// downloaded list.
Status gpu_search_results_host(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *seqs, size_t num_seqs,
                               const NeedleHipProblem *problems, size_t num_problems, uint32_t threshold, EpilogueJob job,
                               std::vector<NeedleHipSearchResult> *results, uint32_t *failed, std::vector<NeedleHipRun> *runs,
                               size_t *num_runs);

// ---- the incremental index (index.cpp) -------------------------------------------------------------------------------------
// A store in HBM, owned by one NeedleHipIndex: the heap entries of every pair searched so far, per bucket
// b = p(i, j) * regions + r with the column-major pair id p(i, j) = j (j - 1) / 2 + i (an append adds ids at the end), the
// buckets' start / valid counts, the videos' row tables (length, timestamps), hash durations and the hash arena.
struct IndexStore;
IndexStore *index_store_new();  // on the current device
void index_store_free(IndexStore *store);

// DeviceEntry's layout (epilogue.hip), for the entries the host computes when an append falls back (static_assert there)
struct IndexEntry {
  uint64_t src_start, src_end, dst_start, dst_end;
  uint32_t score, src_hash, dst_hash, pad;
};

// One append: videos [n0, n1) join the n0 the store holds.  Rows are video * regions + region.
struct IndexAppend {
  uint32_t n0 = 0, n1 = 0, regions = 1, threshold = 0;
  bool include_endings = false, large_ok = false;
  ns_t min_opening_duration = 0, min_ending_duration = 0, time_padding = 0;
  const uint32_t *hashes = nullptr;  // the new rows' hashes, appended to the arena behind the committed ones
  size_t num_hashes = 0;
  const NeedleHipSeq *seqs = nullptr;  // ALL rows, offsets into the arena after the append
  size_t num_seqs = 0;
  const NeedleHipProblem *problems = nullptr;  // the new pairs only; tag = (p(i, j) - p(0, n0)) * regions + region
  size_t num_problems = 0;
  const uint32_t *row_len = nullptr, *row_ts = nullptr;  // the new rows: length, offset of their timestamps in the store's table
  size_t num_rows = 0;
  const uint64_t *ts = nullptr;  // timestamps appended to the store's table
  size_t num_ts = 0;
  const uint64_t *hash_duration = nullptr;  // per new video
};
struct IndexAppendOut {
  uint32_t found = 0;   // runs the scan found
  uint32_t failed = 0;  // videos whose padding / hash duration exceed the match end, | kEpilogueBucketTooLarge
  uint32_t held = 0;    // (an edit) the heap entries the rebuilt store holds
  std::vector<uint32_t> videos;                 // the videos whose candidate list changed ...
  std::vector<NeedleHipSearchResult> results;   // ... and their new results
  std::vector<NeedleHipRun> runs;               // kEpilogueBucketTooLarge: the append's run list, for the host
};
// Upload, scan of the new pairs, entries into the store, best_match over the changed videos, all on the library stream;
// one wait, for the final copy.  Nothing is committed: the caller does that (index_store_commit) once the results are good.
Status gpu_index_append(IndexStore *store, const IndexAppend &append, IndexAppendOut *out);
// The fallback: the append's new buckets computed on the host (start[b] relative to the append's first entry, valid[b],
// the entries), uploaded into the store; then best_match as above.
Status gpu_index_append_host_entries(IndexStore *store, const IndexAppend &append, const std::vector<uint32_t> &start,
                                     const std::vector<uint32_t> &valid, const std::vector<IndexEntry> &entries, IndexAppendOut *out);
void index_store_commit(IndexStore *store, const IndexAppend &append, uint32_t entries_written);

// One removal or replacement: the store is rebuilt for a new list of n_new videos, each an old video kept in place of its
// relative order (old_of_new[v] = its old position) or a fresh one (kIndexFresh: a replacement).  Pair ids are renumbered,
// so every table is gathered into a second set of buffers; the committed ones are not written (index_store_switch makes
// the new ones current).  Rows are video * regions + region.
constexpr uint32_t kIndexFresh = 0xFFFFFFFFu;
struct IndexSegment {  // a kept row: `len` elements from `src` in the committed table to `dst` in the new one
  uint64_t src, dst, len;
};
struct IndexEdit {
  uint32_t n_old = 0, n_new = 0, regions = 1, threshold = 0;
  bool include_endings = false, large_ok = false;
  ns_t min_opening_duration = 0, min_ending_duration = 0, time_padding = 0;
  const uint32_t *old_of_new = nullptr;  // [n_new]: the old position, or kIndexFresh
  const uint32_t *new_of_old = nullptr;  // [n_old]: the new position of a video kept, or kIndexFresh (removed or replaced)
  const uint32_t *gone = nullptr;        // the old positions removed or replaced: their pairs' entries are dropped
  size_t num_gone = 0;
  const IndexSegment *hash_rows = nullptr, *ts_rows = nullptr;  // the kept rows' hashes and (distinct) timestamp runs
  size_t num_hash_rows = 0, num_ts_rows = 0;
  const uint32_t *hashes = nullptr;  // the fresh rows' hashes, behind the kept ones: the arena then holds total_hashes
  size_t num_hashes = 0;
  uint64_t total_hashes = 0;
  const uint64_t *ts = nullptr;  // the fresh rows' own timestamps, behind the kept ones: the table then holds total_ts
  size_t num_ts = 0;
  uint64_t total_ts = 0;
  const NeedleHipSeq *seqs = nullptr;  // every new row
  const uint32_t *row_len = nullptr, *row_ts = nullptr;  // every new row
  const uint64_t *hash_duration = nullptr;               // every new video
  const NeedleHipProblem *problems = nullptr;  // the pairs with a fresh video; tag = listed pair * regions + region
  size_t num_problems = 0;
  const uint32_t *pair_ids = nullptr;  // listed pair -> its new id p(i, j)
  size_t num_pairs = 0;
};
// As gpu_index_append: upload, the new tables gathered, the scan of the listed pairs, their entries behind the committed
// ones, every bucket gathered into the second entry buffer (no dead slots), best_match over the videos whose candidate
// list changed; one wait.  out->held: the entries the rebuilt store holds.
Status gpu_index_edit(IndexStore *store, const IndexEdit &edit, IndexAppendOut *out);
// The fallback: the listed buckets computed on the host (start[b] relative to the first fresh entry, valid[b], entries).
Status gpu_index_edit_host_entries(IndexStore *store, const IndexEdit &edit, const std::vector<uint32_t> &start,
                                   const std::vector<uint32_t> &valid, const std::vector<IndexEntry> &entries, IndexAppendOut *out);
void index_store_switch(IndexStore *store, const IndexEdit &edit, uint32_t held);
void index_store_clear(IndexStore *store);  // every video removed (no device work)
// [0] heap entries held (sum of the buckets' valid counts: one read of the table), [1] entry slots in use, [2] hashes in
// the arena, [3] timestamps in the table.
Status index_store_sizes(IndexStore *store, uint64_t sizes[4]);

}  // namespace needle
