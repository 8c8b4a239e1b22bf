// The host side of a round of the streaming comparators (matcher.hip, crossmatch.hip; the device side is stream_walk.h):
// the round's one upload, the run slab with its one download, what comes from a feeder, and the poison rule.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "feeder.h"
#include "hipctx.h"

namespace needle {

// The runs of a round: the counter in word 0, the runs from byte 32.  The counter and the first 127 runs come down in one
// copy, the rest, if any, in a second one.  A round writes no state that it reads, so when more runs were counted than the
// slab holds nothing is lost: the slab grows to what was counted and the caller runs the same launches again.
template <typename Run>
struct RunSlab {
  static constexpr uint32_t kHeaderWords = 8, kHeadRuns = 127;
  DeviceBuffer<uint32_t> slab;
  PinnedStage head_stage;
  uint32_t capacity = 4096;  // runs the slab holds

  void capacity_from_env(const char *name) {
    if (const char *e = getenv(name)) capacity = (uint32_t)std::min<long long>(std::max(1ll, atoll(e)), 1ll << 26);
  }
  uint64_t bytes() const { return kHeaderWords * 4 + (uint64_t)capacity * sizeof(Run); }

  // Before the launches (of every repeat): where the land kernel clears the counter and the walk puts the runs.
  Status begin(uint32_t **d_count, Run **d_runs) {
    Status s = slab.reserve(kHeaderWords + (uint64_t)capacity * (sizeof(Run) / 4));
    if (s.ok()) *d_count = slab.ptr, *d_runs = reinterpret_cast<Run *>(slab.ptr + kHeaderWords);
    return s;
  }
  // After them: synchronises the stream.  *retry: the slab was too small and is larger now, `got` is untouched.
  Status collect(hipStream_t stream, std::vector<Run> *got, bool *retry) {
    const uint32_t head = std::min(capacity, kHeadRuns);
    const size_t head_bytes = kHeaderWords * 4 + (size_t)head * sizeof(Run);
    Status s = head_stage.acquire(head_bytes);
    if (!s.ok()) return s;
    NEEDLE_HIP_TRY(hipMemcpyAsync(head_stage.ptr, slab.ptr, head_bytes, hipMemcpyDeviceToHost, stream));
    NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
    const uint32_t found = *static_cast<const uint32_t *>(head_stage.ptr);
    if ((*retry = found > capacity)) {
      capacity = std::max(found, capacity * 2);
      return Status::Ok();
    }
    got->resize(found);
    const uint32_t first = std::min(found, head);
    if (first) std::memcpy(got->data(), static_cast<const char *>(head_stage.ptr) + kHeaderWords * 4, (size_t)first * sizeof(Run));
    if (found > first) {
      const Run *d_runs = reinterpret_cast<const Run *>(slab.ptr + kHeaderWords);
      NEEDLE_HIP_TRY(hipMemcpy(got->data() + first, d_runs + first, (size_t)(found - first) * sizeof(Run), hipMemcpyDeviceToHost));
    }
    return Status::Ok();
  }
};

// The round's one upload: the lane table, then the pieces' items where the table's stage_off says (in words; `words` in
// all), through `stage`.  lanes[i] belongs to pieces[i]; a Lane has stage_off, a Piece items and width.
template <typename Lane, typename Piece>
Status upload_round(const std::vector<Lane> &lanes, const std::vector<Piece> &pieces, uint64_t words, DeviceBuffer<uint32_t> *d_round,
                    PinnedStage *stage, hipStream_t stream) {
  Status s = d_round->reserve(words);
  if (!s.ok() || !(s = stage->acquire(words * 4)).ok()) return s;
  std::memcpy(stage->ptr, lanes.data(), lanes.size() * sizeof(Lane));
  for (size_t i = 0; i < lanes.size(); i++)
    if (pieces[i].width) std::memcpy(static_cast<uint32_t *>(stage->ptr) + lanes[i].stage_off, pieces[i].items, (size_t)pieces[i].width * 4);
  NEEDLE_HIP_TRY(hipMemcpyAsync(d_round->ptr, stage->ptr, words * 4, hipMemcpyHostToDevice, stream));
  stage->mark(stream);
  return Status::Ok();
}

// A failed round poisons the object unless it refused its arguments: then nothing has moved.
inline Status poison_on_failure(const Status &s, Status *poison) {
  if (!s.ok() && s.code != NeedleError_InvalidArgument && s.code != NeedleError_NullArgument) *poison = s;
  return s;
}

// What a feeder holds beyond what `lanes` lanes have taken: the arguments of a Feed, and the lanes to finish after it.
struct FeederTake {
  std::vector<std::vector<uint32_t>> taken;
  std::vector<const uint32_t *> ptrs;
  std::vector<size_t> counts, finish;
};
// lane_state(i, &fed, &finished) reads a lane; `who` is the prefix of the messages ("matcher: "), `finished_hint` what its
// object adds to "the lane is finished", the answer of a finished lane when the feeder has gone on.
template <typename LaneState>
Status take_from_feeder(Feeder *feeder, size_t lanes, const Status &poison, const LaneState lane_state, const std::string &who,
                        const char *finished_hint, FeederTake *out) {
  if (!feeder) return Status::Make(NeedleError_NullArgument, who + "null argument");
  if (feeder->lanes() != lanes) return Status::Make(NeedleError_InvalidArgument, who + "the feeder has another number of lanes");
  if (!poison.ok()) return poison;
  out->taken.assign(lanes, {});
  out->ptrs.assign(lanes, nullptr);
  out->counts.assign(lanes, 0);
  for (size_t i = 0; i < lanes; i++) {
    size_t kept = 0;
    bool finished = false, lane_finished = false;
    uint64_t fed = 0;
    Status s = feeder->Ready(i, &kept, nullptr, &finished);
    if (!s.ok()) return s;
    lane_state(i, &fed, &lane_finished);
    if (lane_finished) {
      if (kept != fed || !finished) return Status::Make(NeedleError_InvalidArgument, who + "the lane is finished" + finished_hint);
      continue;
    }
    if (kept < fed) return Status::Make(NeedleError_InvalidArgument, who + "the feeder's lane holds fewer items than the matcher has taken");
    out->taken[i].resize(kept - fed);
    if (!out->taken[i].empty() && !(s = feeder->Items(i, (size_t)fed, out->taken[i].size(), out->taken[i].data())).ok()) return s;
    out->ptrs[i] = out->taken[i].data();
    out->counts[i] = out->taken[i].size();
    if (finished) out->finish.push_back(i);
  }
  return Status::Ok();
}

}  // namespace needle
