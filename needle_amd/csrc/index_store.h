// The device store of the incremental index (index_store.hip; the host side is index.cpp).
#pragma once

#include <vector>

#include "epilogue.h"
#include "pair_ids.h"

namespace needle {

// A store in HBM, owned by one NeedleHipIndex: the heap entries of every pair searched so far, per bucket
// b = p(i, j) * regions + r with the column-major pair id p(i, j) = j (j - 1) / 2 + i (an append adds ids at the end), the
// buckets' start / valid counts, the videos' row tables (length, timestamps), hash durations and the hash arena.  A grouped
// index (IndexOptions::groups) holds only the pairs inside a group, under pair_ids.h's IndexGroupView ids, and the tables of
// its current list beside the others.
struct IndexStore;
IndexStore *index_store_new();  // on the current device
void index_store_free(IndexStore *store);

// DeviceEntry's layout (epilogue_kernels.h), for the entries the host computes when an append falls back (static_assert in index_store.hip)
struct IndexEntry {
  uint64_t src_start, src_end, dst_start, dst_end;
  uint32_t score, src_hash, dst_hash, pad;
};

struct IndexSegment {  // `len` elements at `src` of one table and at `dst` of another (an edit's kept rows: committed -> new)
  uint64_t src, dst, len;
};

struct IndexOptions : EpilogueOptions {  // of an append or an edit
  bool large_ok = false;  // after it, every row is under 65 536 hashes and its timestamps strictly increase
  // A grouped index: the tables of the list AFTER the operation, built by the caller.  Pair ids are then
  // pair_ids.h's IndexGroupView ids -- only pairs inside a group exist, an append's new ids are [vbase[n0], vbase[n1]) -- and
  // the store uploads the tables beside its own and makes them the committed ones with index_store_commit / _switch.  Null: a
  // plain index, column-major ids, none of the grouped kernels.
  const IndexGroupTables *groups = nullptr;
};

// One append: videos [n0, n1) join the n0 the store holds.  Rows are video * regions + region.
struct IndexAppend : IndexOptions {
  uint32_t n0 = 0, n1 = 0;
  const uint32_t *hashes = nullptr;  // the new rows' hashes, appended to the arena behind the committed ones
  size_t num_hashes = 0;
  const NeedleHipSeq *seqs = nullptr;  // ALL rows, offsets into the arena after the append
  size_t num_seqs = 0;
  const NeedleHipProblem *problems = nullptr;  // the new pairs only; tag = (p(i, j) - p(0, n0)) * regions + region (grouped: id - vbase[n0])
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
  uint32_t refused = 0;                         // (gpu_index_append_matched) kIngest* bits: the matcher's runs or hashes do not fit the rows
};
// Upload, scan of the new pairs, entries into the store, best_match over the changed videos, all on the library stream;
// one wait, for the final copy.  Nothing is committed: the caller does that (index_store_commit) once the results are good.
Status gpu_index_append(IndexStore *store, const IndexAppend &append, IndexAppendOut *out);
// The fallback: the append's new buckets computed on the host (start[b] relative to the append's first entry, valid[b],
// the entries), uploaded into the store; then best_match as above.
Status gpu_index_append_host_entries(IndexStore *store, const IndexAppend &append, const std::vector<uint32_t> &start,
                                     const std::vector<uint32_t> &valid, const std::vector<IndexEntry> &entries, IndexAppendOut *out);
void index_store_commit(IndexStore *store, const IndexAppend &append, uint32_t entries_written);

// The same append fed from a complete cross-matcher over the store's videos and the new ones in place of the scan: its run
// list (host; problem = the i-major pair over all n1 videos * regions + region, needle_hip.h) goes up once and one kernel
// leaves what the scan would have left, tagged for the append (pair_ids.h), less the runs the scan's problems exclude (a row
// whose min_len is 0, a run shorter than the pair's max(min_len)).  Everything behind that is gpu_index_append's second half,
// the fallback included (out->runs is then the ingested list).  The new rows are compared with the matcher's histories on the
// device.  out->refused != 0: nothing is to be committed.
struct IndexMatched {
  const NeedleHipRun *runs = nullptr;
  size_t num_runs = 0;
  const uint32_t *min_len = nullptr;      // ALL rows after the append
  const uint32_t *history = nullptr;      // device: the matcher's lane histories
  const IndexSegment *lanes = nullptr;    // a new row: `len` hashes at `src` in the arena after the append, at `dst` in `history`
  size_t num_lanes = 0;
};
constexpr uint32_t kIngestBadRun = 1u;       // a run outside its rows, of an old pair or of no pair
constexpr uint32_t kIngestOtherHashes = 2u;  // a new row's hashes are not what its lane was fed
Status gpu_index_append_matched(IndexStore *store, const IndexAppend &append, const IndexMatched &matched, IndexAppendOut *out);
// The same append fed from TWO run lists (Index::add_streamed), for an index too large for one cross-matcher: the runs of a
// matcher made from the store's rows (Index::matcher) stand in for the resident x arriving pairs, those of a complete
// cross-matcher over the k = n1 - n0 arriving videos alone for the arriving x arriving pairs.  `runs` holds the matcher's
// lanes' lists one after the other (problem = resident video * regions + region; run_lane[q] = the lane of run q, arriving
// video * regions + region), then the cross-matcher's (problem = the i-major pair over the k videos * regions + region).  One
// kernel re-tags both for the append (pair_ids.h: (resident, n0 + t, r) and (n0 + a, n0 + b, r)) and drops what the scan's
// problems exclude, as above; a run outside its rows, of a source or lane that is none, or of another region than its lane's
// sets kIngestBadRun.  Every new row is compared with the history of each object that has one for its lane.
struct IndexLaneRow {  // a new row: `len` hashes at `src` in the arena after the append, and on the device at `history`
  uint64_t src;
  const uint32_t *history;
  uint64_t len;
};
struct IndexStreamed {
  const NeedleHipRun *runs = nullptr;
  size_t num_matcher_runs = 0, num_cross_runs = 0;
  const uint32_t *run_lane = nullptr;   // [num_matcher_runs]
  const uint32_t *min_len = nullptr;    // ALL rows after the append
  const IndexLaneRow *lanes = nullptr;  // up to two per new row (the matcher's history, the cross-matcher's)
  size_t num_lanes = 0;
};
Status gpu_index_append_streamed(IndexStore *store, const IndexAppend &append, const IndexStreamed &streamed, IndexAppendOut *out);
// The committed hash arena on the device (row offsets: IndexRows::seqs), for a cross-matcher's resident rows; null while empty.
// Valid until the next operation on the store.
Status index_store_arena(IndexStore *store, const uint32_t **d_hashes);
int index_store_device(const IndexStore *store);  // the device that was current when the store was made

// One removal or replacement: the store is rebuilt for a new list of n_new videos, each an old video kept in place of its
// relative order (old_of_new[v] = its old position) or a fresh one (kIndexFresh: a replacement).  Pair ids are renumbered,
// so every table is gathered into a second set of buffers; the committed ones are not written (index_store_switch makes
// the new ones current).  Rows are video * regions + region.
constexpr uint32_t kIndexFresh = 0xFFFFFFFFu;
struct IndexEdit : IndexOptions {
  uint32_t n_old = 0, n_new = 0;
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
  const uint32_t *pair_ids = nullptr;  // listed pair -> its new id p(i, j) (grouped: its id under `groups`)
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
// Match evidence (needle_hip.h NeedleHipSearchEvidence), one record per committed video into evidence[0 .. n): best_match over
// EVERY video of the committed store with the winners' index, count and score written out (the third video policy,
// epilogue_kernels.h; a grouped index: its grouped counterpart over the committed tables, options.groups only says so), then
// match_evidence_kernel, which finds the entries behind them.  Reads the committed tables, writes
// the operations' scratch (candidate pool, links, control words) and buffers of its own; one wait.  Nothing is kept.
Status gpu_index_evidence(IndexStore *store, const IndexOptions &options, NeedleHipSearchEvidence *evidence);
// [0] heap entries held (sum of the buckets' valid counts: one read of the table), [1] entry slots in use, [2] hashes in
// the arena, [3] timestamps in the table.
Status index_store_sizes(IndexStore *store, uint64_t sizes[4]);

}  // namespace needle
