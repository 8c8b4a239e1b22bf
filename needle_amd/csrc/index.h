// NeedleHipIndex (index.cpp): an incremental search index that searches only the pairs an append adds.
#pragma once

#include <vector>

#include "needle_core.h"

namespace needle {

struct IndexStore;

struct IndexRows {  // per row (video * regions + region), and the sizes of the device tables the rows point into
  std::vector<NeedleHipSeq> seqs;        // its hashes in the device arena
  std::vector<uint32_t> min_len;         // the shortest run that can pass the duration test (0: none)
  std::vector<uint32_t> row_ts;          // offset of its timestamps in the store's table
  std::vector<uint8_t> row_ok;           // under 65 536 hashes, timestamps strictly increasing ...
  bool large_ok = true;                  // ... and every row is
  uint64_t hashes = 0, ts = 0;           // sizes of the device arena and timestamp table
  explicit IndexRows(size_t rows = 0) : seqs(rows), min_len(rows), row_ts(rows), row_ok(rows) {}
};

// Results equal Comparator::run_with_frame_hashes over the index's current list: the videos added, in insertion order, less
// those removed, with replacements in place.  The index runs on
// the device that was current when it was created; one GPU only (no sharding across ranks).
class Index {
 public:
  explicit Index(const Comparator &comparator);  // copies the comparator's parameters: later changes to it do not matter
  ~Index();
  Index(const Index &) = delete;
  Index &operator=(const Index &) = delete;
  Status init();
  size_t size() const { return videos_.size(); }
  // Appends the videos (copied); on failure the index is as it was before the call.
  Status add(const std::vector<const FrameHashesData *> &videos);
  // Removes the videos at these distinct positions (the others keep their order) / replaces them in place (copied).  The
  // results then equal run_with_frame_hashes over the new list; on failure the index is as it was before the call.
  Status remove(const std::vector<size_t> &positions);
  Status replace(const std::vector<size_t> &positions, const std::vector<const FrameHashesData *> &videos);
  // heap entries held, entry slots in use, hashes in the arena, timestamps in the table
  Status store_sizes(uint64_t sizes[4]) const;
  const std::vector<NeedleHipSearchResult> &results() const { return results_; }
  uint64_t pairs_total() const { return pairs_total_; }
  uint64_t pairs_last() const { return pairs_last_; }

 private:
  Comparator cmp_;  // a copy: its parameters, and entries_from_runs for the host fallback
  bool include_endings_;
  uint32_t regions_;
  IndexStore *store_ = nullptr;
  std::vector<FrameHashesData> videos_;
  IndexRows rows_;
  std::vector<NeedleHipSearchResult> results_;
  uint64_t pairs_total_ = 0, pairs_last_ = 0;

  // remove / replace: the new list is old_of_new[v] (an old position) or, where that is kIndexFresh, *fresh[v]
  Status rebuild(const std::vector<uint32_t> &old_of_new, const std::vector<const FrameHashesData *> &fresh);
};

}  // namespace needle
