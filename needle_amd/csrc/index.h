// NeedleHipIndex (index.cpp): an incremental search index that searches only the pairs an append adds.
#pragma once

#include <vector>

#include "needle_core.h"

namespace needle {

struct IndexStore;

// Results equal Comparator::run_with_frame_hashes over all videos added so far, in insertion order.  The index runs on
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
  const std::vector<NeedleHipSearchResult> &results() const { return results_; }
  uint64_t pairs_total() const { return pairs_total_; }
  uint64_t pairs_last() const { return pairs_last_; }

 private:
  Comparator cmp_;  // a copy: its parameters, and entries_from_runs for the host fallback
  bool include_endings_;
  uint32_t regions_;
  IndexStore *store_ = nullptr;
  std::vector<FrameHashesData> videos_;
  std::vector<NeedleHipSeq> seqs_;        // per row: its hashes in the device arena
  std::vector<uint32_t> min_len_;         // per row: the shortest run that can pass the duration test (0: none)
  std::vector<uint32_t> row_ts_;          // per row: offset of its timestamps in the store's table
  uint64_t hashes_ = 0, ts_ = 0;          // sizes of the device arena and timestamp table
  bool large_ok_ = true;                  // every row under 65 536 hashes, timestamps strictly increasing
  std::vector<NeedleHipSearchResult> results_;
  uint64_t pairs_total_ = 0, pairs_last_ = 0;
};

}  // namespace needle
