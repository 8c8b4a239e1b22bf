// Streaming fingerprinter: chromaprint's start / feed / finish, batched over lanes, with the per-lane state on the
// device (feeder.hip; include/needle_hip.h needle_hip_feeder_*).
#pragma once

#include <memory>

#include "common.h"

namespace needle {

// Kept items a lane holds after `samples` samples per channel: host arithmetic only.  Unfinished, the first pass has
// seen the whole frame PAIRS of the samples fed (a trailing odd frame waits for its partner); finished, every frame.
size_t feeder_num_ready(uint64_t samples, int sample_rate, int channels, uint32_t step, bool finished);
// The same after a stream of several segments (SwitchFormat): every segment but an open last one is resampled whole.
size_t feeder_num_ready_segments(const NeedleHipSegment *segments, size_t count, uint32_t step, bool finished);

class Feeder {
 public:
  static Status Create(size_t lanes, int channels, int sample_rate, int format, uint32_t step, std::unique_ptr<Feeder> *out);
  // Every lane in a format of its own (needle_hip_feeder_new_lanes): such a feeder down-mixes every lane to mono as it
  // lands (feeder_ingest_kernel), so its tails are mono whatever the channel count, and ResetFormat may give a lane
  // another format with its next stream.  Create's feeder keeps one format and refuses ResetFormat.
  static Status CreateLanes(const NeedleHipLaneFormat *formats, size_t lanes, uint32_t step, std::unique_ptr<Feeder> *out);
  Status LaneFormat(size_t lane, NeedleHipLaneFormat *format) const;
  Status ResetFormat(const size_t *lanes, const NeedleHipLaneFormat *formats, size_t k);
  // lanes[j] folds its channels with mixes[j] (channels == 0: the plain average again): CreateLanes' feeder only, and
  // only lanes that hold no samples; all checked before any lane changes.  ResetFormat clears a lane's mix.  While any
  // lane has a mix, a round lands its staged spans with rematrix_kernel instead of feeder_ingest_kernel.
  Status SetLaneMix(const size_t *lanes, const NeedleHipChannelMix *mixes, size_t k);
  // lanes[j] ends its open segment and goes on with ITS SAME STREAM in formats[j] (mixes null or channels == 0: the plain
  // average): CreateLanes' feeder only; every lane, format and mix checked before any lane changes.  The segments that
  // resample and hold samples are flushed by one round without chunks: their last tiles computed with the end known
  // (the segment's, not the lane's: frames stay even), then the source tails dropped.  Other switches launch nothing.
  Status SwitchFormat(const size_t *lanes, const NeedleHipLaneFormat *formats, const NeedleHipChannelMix *mixes, size_t k);
  // the segments of the lane's current stream, the open one last: *count of them, at most `cap` written
  Status LaneSegments(size_t lane, NeedleHipSegment *out, size_t cap, size_t *count) const;
  ~Feeder();
  size_t lanes() const;
  uint32_t step() const;
  // pcm: lane after lane, each lane's sample_format_planes() pointers; num_values[i] values (whole frames) of lane i
  Status Feed(const void *const *pcm, const size_t *num_values);
  Status Finish(const size_t *lanes, size_t k);  // nullptr: every unfinished lane
  Status Reset(const size_t *lanes, size_t k);   // nullptr: every lane
  // these wait for outstanding device work
  Status Ready(size_t lane, size_t *kept_items, uint64_t *samples_fed, bool *finished);
  Status Items(size_t lane, size_t first, size_t count, uint32_t *items);
  Status FinishedItems(size_t lane, const std::vector<uint32_t> **items);  // InvalidArgument unless the lane is finished
  void StateBytes(uint64_t bytes[2]) const;
  // The audit of the f32 first pass, travelling with the stream (needle_hip_feeder_set_audit / _audit).  SetAudit: only
  // while no lane holds samples.  Audit: counts = {items, accepted, accepted mismatches, mismatches} of a lane's current
  // stream, or of all lanes (SIZE_MAX: counts summed, maxima taken); waits for the library stream.
  Status SetAudit(bool on);
  Status Audit(size_t lane, uint64_t counts[4], double *max_ratio, double *max_sigma);

 private:
  Feeder();
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace needle
