// Streaming all-pairs comparator: N lanes whose hashes arrive in chunks, matched against each other; the L-shaped frontier
// of every pair's evaluated rectangle carried in HBM between feeds (crossmatch.hip; include/needle_hip.h
// needle_hip_crossmatcher_*).  With regions the lanes are videos x regions (lane = video * regions + region: openings and
// endings), matched within a region only, each region with its own capacity and min_len.
#pragma once

#include <memory>
#include <vector>

#include "common.h"
#include "feeder.h"

namespace needle {

class CrossMatcher {
 public:
  // Argument checks first, then the device: state and histories are allocated here, so without a device this fails.
  static Status Create(size_t lanes, size_t max_items, uint32_t min_len, uint32_t threshold, std::unique_ptr<CrossMatcher> *out);
  // regions 1 or 2; max_items and min_len hold one entry per region.  Create is the one-region case.
  static Status CreateRegions(size_t videos, size_t regions, const size_t *max_items, const uint32_t *min_len, uint32_t threshold,
                              std::unique_ptr<CrossMatcher> *out);
  // Resident videos: `resident` holds num_resident * regions rows of the arena `hashes` (row k * regions + r), complete
  // and uploaded here; they come before the arriving videos in the video list, and only pairs with an arriving end are
  // live.  Lanes, `videos()` and the feeds are the arriving videos'.  num_resident == 0 is CreateRegions.
  static Status CreateResident(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *resident, size_t num_resident, size_t videos,
                               size_t regions, const size_t *max_items, const uint32_t *min_len, uint32_t threshold,
                               std::unique_ptr<CrossMatcher> *out);
  // The same object with `hashes` an arena in DEVICE memory (the index store's): the rows are gathered into the histories
  // by one launch, no hashes are uploaded; only the resident table goes up.
  static Status CreateResidentDevice(const uint32_t *d_hashes, size_t num_hashes, const NeedleHipSeq *resident, size_t num_resident,
                                     size_t videos, size_t regions, const size_t *max_items, const uint32_t *min_len, uint32_t threshold,
                                     std::unique_ptr<CrossMatcher> *out);
  // Groups: a label per resident and per arriving video (any values, only compared); the live pairs are the same-label ones
  // with an arriving end, and NeedleHipRun.problem is the grouped pair id of pair_ids.h over the K + N labels, x regions +
  // region.  The live-pair table (cross_pairs.h) is uploaded here; state and hashes exist for live pairs only.
  static Status CreateGrouped(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *resident, size_t num_resident,
                              const uint32_t *resident_groups, size_t videos, const uint32_t *groups, size_t regions, const size_t *max_items,
                              const uint32_t *min_len, uint32_t threshold, std::unique_ptr<CrossMatcher> *out);
  // ... with `hashes` an arena in DEVICE memory, as CreateResidentDevice
  static Status CreateGroupedDevice(const uint32_t *d_hashes, size_t num_hashes, const NeedleHipSeq *resident, size_t num_resident,
                                    const uint32_t *resident_groups, size_t videos, const uint32_t *groups, size_t regions,
                                    const size_t *max_items, const uint32_t *min_len, uint32_t threshold, std::unique_ptr<CrossMatcher> *out);
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
  // pairs x 2 sets x 2 (col, row) x max_items x (2 or 4) + lanes x max_items x 4; 0 where the arguments are out of range
  static size_t StateBytes(size_t lanes, size_t max_items);
  // the sum of that over the regions, with one entry width: 2 where every region's max_items < 65 536, else 4
  static size_t StateBytesRegions(size_t videos, size_t regions, const size_t *max_items);
  // with resident rows: per region also videos x 2 sets x S x (2 or 4) + S x 4, S = the region's resident hashes; the width
  // is 4 as soon as one max_items or one resident row reaches 65 536
  static size_t StateBytesResident(const NeedleHipSeq *resident, size_t num_resident, size_t videos, size_t regions, const size_t *max_items);

  // The argument checks of creation without the arena's bounds and without a device: null where they pass, else what to say.
  static const char *ShapeError(const NeedleHipSeq *resident, size_t num_resident, size_t videos, size_t regions, const size_t *max_items,
                                const uint32_t *min_len);

  // what CreateGrouped allocates for frontiers and hashes (cross_pairs.h); 0 where the arguments are refused
  static size_t StateBytesGrouped(const NeedleHipSeq *resident, size_t num_resident, const uint32_t *resident_groups, size_t videos,
                                  const uint32_t *groups, size_t regions, const size_t *max_items);
  // ShapeError for CreateGrouped
  static const char *GroupedShapeError(const NeedleHipSeq *resident, size_t num_resident, const uint32_t *resident_groups, size_t videos,
                                       const uint32_t *groups, size_t regions, const size_t *max_items, const uint32_t *min_len);
  bool grouped() const;
  const std::vector<uint32_t> &labels() const;  // a grouped object's, of all K + N videos, residents first

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
  static Status CreateFrom(const uint32_t *hashes, bool on_device, size_t num_hashes, const NeedleHipSeq *resident, size_t num_resident,
                           size_t videos, size_t regions, const size_t *max_items, const uint32_t *min_len, uint32_t threshold,
                           std::unique_ptr<CrossMatcher> *out);
  static Status CreateGroupedFrom(const uint32_t *hashes, bool on_device, size_t num_hashes, const NeedleHipSeq *resident, size_t num_resident,
                                  const uint32_t *resident_groups, size_t videos, const uint32_t *groups, size_t regions,
                                  const size_t *max_items, const uint32_t *min_len, uint32_t threshold, std::unique_ptr<CrossMatcher> *out);
  CrossMatcher();
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace needle
