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
  ~Matcher();
  size_t lanes() const;
  Status Feed(const uint32_t *const *items, const size_t *num_items);
  Status FeedFromFeeder(Feeder *feeder);
  Status Finish(const size_t *lanes, size_t k);  // nullptr: every unfinished lane
  Status Reset(const size_t *lanes, size_t k);   // nullptr: every lane
  Status Ready(size_t lane, size_t *num_runs, uint64_t *items_fed, bool *finished);
  Status Runs(size_t lane, size_t first, size_t count, NeedleHipRun *runs);
  Status Open(size_t lane, std::vector<NeedleHipRun> *runs);
  void Stats(uint64_t stats[4]) const;  // feeds, kernel launches, cells evaluated, state bytes

 private:
  Matcher();
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace needle
