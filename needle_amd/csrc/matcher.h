// Streaming comparator: S source sequences resident on the device, N lanes whose destination hashes arrive in chunks,
// per-diagonal run lengths carried in HBM between feeds (matcher.hip; include/needle_hip.h needle_hip_matcher_*).
#pragma once

#include <memory>
#include <vector>

#include "common.h"
#include "feeder.h"

namespace needle {

class Matcher {
 public:
  // Argument checks first, then the device: the sources are uploaded here, so without a device this fails.
  static Status Create(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len,
                       size_t num_sources, size_t lanes, uint32_t threshold, std::unique_ptr<Matcher> *out);
  // Regions 1 or 2: source s is in region s % regions, lane l in region l % regions, and a lane meets its own region's sources
  // only.  A source with min_len == 0 is allowed here and, like one shorter than 2 hashes, has no cells.  regions == 1 with
  // every min_len >= 1 is Create.
  static Status CreateRegions(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len,
                              size_t num_sources, size_t regions, size_t lanes, uint32_t threshold, std::unique_ptr<Matcher> *out);
  // The same object with `d_hashes` an arena in DEVICE memory (the index store's): the sources that have cells are gathered into
  // the matcher's own arena by one launch, no hashes are uploaded; only the tables go up.
  static Status CreateRegionsDevice(const uint32_t *d_hashes, size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len,
                                    size_t num_sources, size_t regions, size_t lanes, uint32_t threshold, std::unique_ptr<Matcher> *out);
  // The argument checks of CreateRegions without a device and without the hashes.
  static Status CheckShape(size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len, size_t num_sources, size_t regions,
                           size_t lanes);
  ~Matcher();
  size_t lanes() const;
  size_t regions() const;
  Status Feed(const uint32_t *const *items, const size_t *num_items);
  Status FeedFromFeeder(Feeder *feeder);
  Status Finish(const size_t *lanes, size_t k);  // nullptr: every unfinished lane
  Status Reset(const size_t *lanes, size_t k);   // nullptr: every lane
  Status Ready(size_t lane, size_t *num_runs, uint64_t *items_fed, bool *finished);
  Status Runs(size_t lane, size_t first, size_t count, NeedleHipRun *runs);
  Status Open(size_t lane, std::vector<NeedleHipRun> *runs);
  void Stats(uint64_t stats[4]) const;  // feeds, kernel launches, cells evaluated, state bytes

  // What an index needs of a matcher it made (Index::matcher, Index::add_streamed).
  struct Origin {  // the index and its generation at creation; index_id 0: not made from an index
    uint64_t index_id = 0, generation = 0;
  };
  void set_origin(const Origin &origin);
  Origin origin() const;
  int device() const;       // the device current at creation
  Status poisoned() const;  // the device failure every call returns, or Ok
  const std::vector<NeedleHipRun> &run_list(size_t lane) const;  // what Runs copies from
  const uint32_t *history(size_t lane) const;  // device: the lane's hashes so far, items_fed of them; null where the lane only counts

 private:
  Matcher();
  struct Impl;
  static Status Plan(Impl *impl, bool packed, size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len, bool min_len_zero_ok,
                     size_t num_sources, size_t regions, size_t lanes);
  static Status CreateFrom(const uint32_t *hashes, bool on_device, size_t num_hashes, const NeedleHipSeq *sources, const uint32_t *min_len,
                           bool min_len_zero_ok, size_t num_sources, size_t regions, size_t lanes, uint32_t threshold,
                           std::unique_ptr<Matcher> *out);
  std::unique_ptr<Impl> impl_;
};

}  // namespace needle
