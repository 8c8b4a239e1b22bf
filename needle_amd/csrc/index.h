// NeedleHipIndex (index.cpp): an incremental search index that searches only the pairs an append adds.
#pragma once

#include <memory>
#include <vector>

#include "crossmatch.h"
#include "matcher.h"
#include "index_plan.h"
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
// A GROUPED index holds a library of many seasons: every video has a label, equal labels are one season, only
// pairs inside a season are searched, and the results equal run_with_frame_hashes over each season's own sub-list of the
// current list.  It is made as such: labels are given with every add and kept by remove and replace.
class Index {
 public:
  // copies the comparator's parameters: later changes to it do not matter
  explicit Index(const Comparator &comparator, bool grouped = false);
  ~Index();
  Index(const Index &) = delete;
  Index &operator=(const Index &) = delete;
  Status init();
  size_t size() const { return videos_.size(); }
  // Appends the videos (copied); on failure the index is as it was before the call.
  Status add(const std::vector<const FrameHashesData *> &videos);
  // ... with a label per video (any values: they are only compared), on a grouped index: the pairs searched are each arriving
  // video's with the members of its group before it in the list.  add() without labels on a grouped index, labels on a plain
  // one and the four streamed routes below on a grouped one are InvalidArgument, before any device work.
  Status add_grouped(const std::vector<const FrameHashesData *> &videos, const uint32_t *labels);
  bool grouped() const { return grouped_; }
  const std::vector<uint32_t> &labels() const { return labels_; }  // the current list's (a grouped index)
  // A cross-matcher over the index's videos (its resident rows, gathered from the store's arena on the device) and `videos`
  // arriving ones, with the index's regions and threshold.  It remembers the index and its generation.
  Status crossmatcher(size_t videos, const size_t *max_items, const uint32_t *min_len, std::unique_ptr<CrossMatcher> *out);
  // add() with the runs of a complete matcher made by crossmatcher() since the last change in place of the scan: the same
  // index afterwards, no pair searched again.  Every check comes before the commit; on failure the index is as it was.
  Status add_matched(CrossMatcher *matcher, const std::vector<const FrameHashesData *> &videos);
  // The grouped index's forms of the two: a grouped cross-matcher (crossmatch.h: a Spec with labels) whose residents are the
  // index's videos under the index's labels and whose `videos` arriving ones carry `groups`; add_matched_grouped appends them
  // under those labels and leaves what add_grouped would.  A plain index: InvalidArgument.
  Status crossmatcher_grouped(size_t videos, const uint32_t *groups, const size_t *max_items, const uint32_t *min_len,
                              std::unique_ptr<CrossMatcher> *out);
  Status add_matched_grouped(CrossMatcher *matcher, const std::vector<const FrameHashesData *> &videos);
  // The second route, for an index too large for one cross-matcher (its live problems are a grid dimension): a matcher whose
  // sources are the index's rows, region-aware, with `videos` * regions lanes; each source's min_len is the row's own.  It
  // remembers the index and its generation.  An empty index has nothing resident: InvalidArgument.
  Status matcher(size_t videos, std::unique_ptr<Matcher> *out);
  // add() with the runs of a complete matcher made by matcher() since the last change in place of the scan of the resident x
  // arriving pairs, and those of a complete cross-matcher over the arriving videos alone (no residents; null with one video) in
  // place of the arriving pairs'.  The same index afterwards; every check comes before the commit.
  Status add_streamed(Matcher *matcher, CrossMatcher *crossmatcher, const std::vector<const FrameHashesData *> &videos);
  // Removes the videos at these distinct positions (the others keep their order) / replaces them in place (copied).  The
  // results then equal run_with_frame_hashes over the new list; on failure the index is as it was before the call.
  Status remove(const std::vector<size_t> &positions);
  Status replace(const std::vector<size_t> &positions, const std::vector<const FrameHashesData *> &videos);
  // heap entries held, entry slots in use, hashes in the arena, timestamps in the table
  Status store_sizes(uint64_t sizes[4]) const;
  const std::vector<NeedleHipSearchResult> &results() const { return results_; }
  // One evidence record per video (needle_hip.h), size() of them, computed on the device from the committed store when
  // asked: best_match over every video with the winners written out, then the entries behind them.  Changes nothing.
  Status evidence(NeedleHipSearchEvidence *out) const;
  uint64_t pairs_total() const { return pairs_total_; }
  uint64_t pairs_last() const { return pairs_last_; }
  // pairs handed to the one-shot scan (add_matched and add_streamed hand it none)
  uint64_t scanned_total() const { return scanned_total_; }
  uint64_t scanned_last() const { return scanned_last_; }

 private:
  Comparator cmp_;  // a copy: its parameters, and entries_from_runs for the host fallback
  bool include_endings_;
  uint32_t regions_;
  IndexStore *store_ = nullptr;
  const bool grouped_;
  std::vector<uint32_t> labels_;            // a grouped index: the current list's labels
  std::unique_ptr<const IndexPairIds> ids_;  // the current list's pair ids (index_plan.h; null while empty)
  std::vector<FrameHashesData> videos_;
  IndexRows rows_;
  std::vector<NeedleHipSearchResult> results_;
  uint64_t pairs_total_ = 0, pairs_last_ = 0, scanned_total_ = 0, scanned_last_ = 0;
  const uint64_t id_;        // from a process-wide counter: what a matcher made here remembers, with ...
  uint64_t generation_ = 1;  // ... this, which every successful change advances

  // every add: `labels` null on a plain index; `cross` and `matcher` as the route has them (index_plan.h)
  Status append(const std::vector<const FrameHashesData *> &videos, const uint32_t *labels, IndexRoute route = IndexRoute::Scan,
                CrossMatcher *cross = nullptr, Matcher *matcher = nullptr);
  // what the route's objects say of themselves, and the index of itself
  IndexAcceptance acceptance(IndexRoute route, size_t k, CrossMatcher *cross, Matcher *matcher) const;
  // crossmatcher (groups null) and crossmatcher_grouped after their own refusals
  Status make_crossmatcher(size_t videos, const uint32_t *groups, const size_t *max_items, const uint32_t *min_len,
                           std::unique_ptr<CrossMatcher> *out);
  Status refuse_grouped(const char *route) const;  // the streamed routes on a grouped index
  void changed(uint64_t searched, uint64_t scanned);  // the counters, at a commit

  // remove / replace: the new list is old_of_new[v] (an old position) or, where that is kIndexFresh, *fresh[v]
  Status rebuild(const std::vector<uint32_t> &old_of_new, const std::vector<const FrameHashesData *> &fresh);
};

}  // namespace needle
