// Streaming all-pairs comparator: N lanes whose hashes arrive in chunks, matched against each other; the L-shaped frontier
// of every pair's evaluated rectangle carried in HBM between feeds (crossmatch.hip; include/needle_hip.h
// needle_hip_crossmatcher_*).  With regions the lanes are videos x regions (lane = video * regions + region: openings and
// endings), matched within a region only, each region with its own capacity and min_len.
#pragma once

#include <memory>
#include <vector>

#include "common.h"
#include "cross_pairs.h"
#include "feeder.h"

namespace needle {

class CrossMatcher {
 public:
  // What the object is made from: resident rows (complete at creation, rows k * regions + r of the caller's arena; they come
  // before the arriving videos in the video list, and only pairs with an arriving end are live), the arriving videos (the lanes,
  // `videos()` and the feeds are theirs), regions 1 or 2 with a max_items and a min_len each, and optionally a label per video:
  // then the live pairs are the same-label ones and NeedleHipRun.problem is the grouped pair id of pair_ids.h over the K + N
  // labels, x regions + region.  cross_pairs.h plans all of them, refusals included.
  using Spec = CrossPairsShape;
  // Argument checks first, then the device: state and histories are allocated here, so without a device this fails.  `hashes`
  // is the arena of the resident rows (num_hashes of them), on the host and uploaded here, or with `on_device` in DEVICE memory
  // (the index store's): the rows are gathered into the histories by one launch, no hashes are uploaded.
  static Status Create(Spec spec, const uint32_t *hashes, size_t num_hashes, bool on_device, std::unique_ptr<CrossMatcher> *out);
  ~CrossMatcher();
  size_t lanes() const;  // videos * regions
  size_t residents() const;
  size_t videos() const;
  size_t regions() const;
  Status Feed(const uint32_t *const *items, const size_t *num_items);
  Status FeedFromFeeder(Feeder *feeder);
  Status Finish(const size_t *lanes, size_t k);  // nullptr: every unfinished lane
  Status Ready(size_t *num_runs, bool *complete);
  Status Lane(size_t lane, uint64_t *items_fed, bool *finished);
  Status Runs(size_t first, size_t count, NeedleHipRun *runs);
  void Stats(uint64_t stats[4]) const;  // feeds, kernel launches, cells evaluated, state bytes
  // what Create allocates for frontiers and hashes (cross_pairs.h; spec.min_len may be null); 0 where the spec is refused
  static size_t StateBytes(const Spec &spec);
  // The argument checks of creation without the arena's bounds and without a device: null where they pass, else what to say.
  static const char *ShapeError(const Spec &spec);
  bool grouped() const;
  const std::vector<uint32_t> &labels() const;  // a grouped object's, of all K + N videos, residents first; else empty

  // What an index needs of a matcher it made (Index::crossmatcher, Index::add_matched).
  struct Origin {  // the index and its generation at creation; index_id 0: not made from an index
    uint64_t index_id = 0, generation = 0;
  };
  void set_origin(const Origin &origin);
  Origin origin() const;
  int device() const;  // the device current at creation
  uint32_t min_len(size_t region) const;
  Status poisoned() const;                             // the device failure every call returns, or Ok
  const std::vector<NeedleHipRun> &run_list() const;   // what Runs copies from
  const uint32_t *history(size_t lane) const;          // device: the lane's hashes so far, items_fed of them

 private:
  CrossMatcher();
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace needle
