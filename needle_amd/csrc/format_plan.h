// The host plan of a library's PCM on its way in, whether every video has the library's one format or a format of its
// own (needle_hip_library_set_video_formats): the walk over the caller's pointer array, and the cut of the windows into
// staged pieces and batches, whatever lands them.  Host arithmetic only --
// no device, no HIP -- so that it can be driven by a stand-alone program (tests/cpp/format_plan_check.cpp).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "common.h"

namespace needle {

// Where video v's planes lie in the concatenation of every video's planes (an interleaved video has one, a planar one
// `channels`): first[v], first[n] = the array's length.
inline std::vector<size_t> format_first_planes(const NeedleHipLaneFormat *formats, size_t n) {
  std::vector<size_t> first(n + 1, 0);
  for (size_t v = 0; v < n; v++) first[v + 1] = first[v] + sample_format_planes(formats[v].format, formats[v].channels);
  return first;
}

// The limits of one video's (stream's, lane's) format and of its mix against it -- channels 1..8, sample_rate
// 2000..768000 with a resampler design, a known sample format, a mix of that channel count -- on the host, no device.
inline Status lane_format_check(const NeedleHipLaneFormat &f, const NeedleHipChannelMix *mix, const std::string &who) {
  if (f.channels < 1 || f.channels > NEEDLE_HIP_MAX_CHANNELS)
    return Status::Make(NeedleError_InvalidArgument, who + ": channels must be 1 to " + std::to_string(NEEDLE_HIP_MAX_CHANNELS));
  if (f.sample_rate < 2000 || f.sample_rate > 768000) return Status::Make(NeedleError_InvalidArgument, who + ": unsupported sample rate");
  if (!sample_format_valid(f.format)) return Status::Make(NeedleError_InvalidArgument, who + ": unknown sample format");
  ResampleTiling tiling;
  if (f.sample_rate != kSampleRate) {
    Status s = resample_tiling_host(f.sample_rate, &tiling);
    if (!s.ok()) return s;
  }
  return mix ? channel_mix_check(*mix, f.channels) : Status::Ok();
}

// A video is held with all its planes or with none: (*held)[v] (optional) says which.  NullArgument for one with both kinds.
inline Status format_walk_planes(const void *const *pcm, const std::vector<size_t> &first, std::vector<char> *held = nullptr) {
  const size_t n = first.size() - 1;
  if (held) held->assign(n, 0);
  for (size_t v = 0; v < n; v++) {
    for (size_t p = first[v] + 1; p < first[v + 1]; p++)
      if (!pcm[p] != !pcm[first[v]])
        return Status::Make(NeedleError_NullArgument, "video " + std::to_string(v) + " has NULL and non-NULL planes");
    if (held) (*held)[v] = pcm[first[v]] != nullptr;
  }
  return Status::Ok();
}

// What lands a window's raw samples as s16 (library.cpp issues the launch): nothing -- interleaved s16 of 1-2 channels is
// read by the resampler, or copied into the resident PCM, as it is --, gpu_downmix_device, gpu_convert_device,
// gpu_rematrix_device or gpu_ingest_device.
enum class Landing { None, Downmix, Convert, Rematrix, Ingest };

// One window this rank holds, in its video's format.
struct FormatWindow {
  const void *src[NEEDLE_HIP_MAX_CHANNELS] = {};  // the planes (one if interleaved) at the window's first frame
  uint64_t frames = 0;
  int channels = 1, format = NEEDLE_HIP_SAMPLE_S16, rate = kSampleRate;
  const NeedleHipChannelMix *mix = nullptr;  // nullptr: the plain average
  uint64_t dst = 0;                          // the window's place in the resident PCM, in s16 values
  Landing landing = Landing::Ingest;
  int out_channels = 1;  // of what the landing writes: 2 only for a 2-channel window of a uniform library without a mix
                         // (Landing::None: of the raw s16 itself, 1 or 2)
};

// A piece of a window: input frames [p0, p1), staged at raw_off (host windows: plane c at raw_off + c * plane_units) and
// landed at mono_off of the staging -- mono, or the 1-2 channels a uniform library's conversion keeps -- (resampled
// windows: output tiles [t0, t1) of the window's rate) or straight in the
// resident PCM at the window's dst + p0 * out_channels.  Offsets in s16 units of the batch's staging buffer.
struct FormatPiece {
  size_t window = 0, batch = 0;
  uint64_t t0 = 0, t1 = 0, p0 = 0, p1 = 0;
  uint64_t raw_off = 0, plane_units = 0, mono_off = 0;
};

struct FormatPlan {
  std::vector<FormatPiece> pieces;  // in window order; a batch is a run of consecutive pieces
  size_t batches = 0;
  uint64_t capacity = 0;  // s16 units of staging any batch needs at most (0: nothing is staged)
};

// The staging limit of a batch in s16 units (2 GiB), or -- NEEDLE_HIP_MAX_BATCH_VALUES, tests -- in values whatever their
// width (*count_values).
inline uint64_t batch_limit(bool *count_values) {
  const char *e = getenv("NEEDLE_HIP_MAX_BATCH_VALUES");
  *count_values = e != nullptr;
  return e ? (uint64_t)std::max(1ll, atoll(e)) : 1ull << 30;
}

// Pieces are whole 16-frame groups or, resampled, whole output tiles of the rate's own tiling (`tilings`: one entry per
// distinct rate other than 11025 Hz) with the input their taps read.  A batch holds at most `limit` s16 units of
// staging or one piece if that is larger.  Staged are the raw planes of a host window, each 16-byte aligned (a device
// window is read in place), and what a landing writes for the resampler to read, out_channels values per frame; a
// window without a landing is resampled out of its raw samples, so a device window of that kind stages nothing and is
// one piece of all its tiles.  A piece is given a quarter of the limit at most, so that a batch goes on filling behind a
// window's last piece with the next window's first ones, whatever their formats.
// `count_values`: the limit counts values whatever their width (batch_limit).
// (A window with neither a landing nor a resampler has nothing to stage and no launch to feed: library.cpp copies it.)
inline Status format_plan_pieces(const std::vector<FormatWindow> &windows, const std::map<int, ResampleTiling> &tilings,
                                 bool from_host, uint64_t limit, bool count_values, FormatPlan *out) {
  out->pieces.clear();
  out->batches = 0;
  out->capacity = 0;
  std::vector<uint64_t> staged;  // per piece
  uint64_t total = 0, largest = 0;
  for (size_t i = 0; i < windows.size(); i++) {
    const FormatWindow &w = windows[i];
    if (w.frames == 0) continue;
    const bool resampled = w.rate != kSampleRate, landed = resampled && w.landing != Landing::None;
    const uint64_t C = (uint64_t)w.channels, OC = (uint64_t)w.out_channels, W = sample_format_width(w.format);
    const uint64_t P = sample_format_planes(w.format, w.channels), per_frame = P == 1 ? C : 1;
    uint64_t budget = ~0ull;  // frames per piece
    const uint64_t piece_limit = std::max<uint64_t>(limit / 4, 1);
    if (from_host || landed)
      budget = count_values ? piece_limit / ((from_host ? C : 0) + (landed ? OC : 0))
                            : 2 * piece_limit / ((from_host ? C * W : 0) + (landed ? 2 * OC : 0));
    const size_t first = out->pieces.size();
    if (resampled) {
      const auto it = tilings.find(w.rate);
      if (it == tilings.end()) return Status::Make(NeedleError_InvalidArgument, "no resampler tiling for rate " + std::to_string(w.rate));
      const ResampleTiling &tl = it->second;
      const uint64_t tile_in = tl.tile_outputs * (uint64_t)tl.M / (uint64_t)tl.L + 2 * (uint64_t)tl.half + 16;  // one tile's input at most
      const uint64_t tiles = (resample_out_len(w.frames, w.rate) + tl.tile_outputs - 1) / tl.tile_outputs;
      const uint64_t piece_tiles = budget == ~0ull ? tiles
                                                   : std::max<uint64_t>(1, (std::max(budget, tile_in) - 2 * (uint64_t)tl.half - 16) *
                                                                               (uint64_t)tl.L / (tl.tile_outputs * (uint64_t)tl.M));
      for (uint64_t t0 = 0; t0 < tiles; t0 += std::min(piece_tiles, tiles - t0)) {
        FormatPiece pc;
        pc.window = i;
        pc.t0 = t0;
        pc.t1 = std::min(tiles, t0 + piece_tiles);
        resample_piece(tl, w.frames, pc.t0, pc.t1, &pc.p0, &pc.p1);
        if (pc.p1 > pc.p0) out->pieces.push_back(pc);
      }
    } else {
      const uint64_t piece_frames = std::max<uint64_t>(16, budget / 16 * 16);
      for (uint64_t f = 0; f < w.frames; f += std::min(piece_frames, w.frames - f)) {
        FormatPiece pc;
        pc.window = i;
        pc.p0 = f;
        pc.p1 = f + std::min(piece_frames, w.frames - f);
        out->pieces.push_back(pc);
      }
    }
    for (size_t k = first; k < out->pieces.size(); k++) {
      FormatPiece &pc = out->pieces[k];
      const uint64_t n = pc.p1 - pc.p0;
      pc.plane_units = from_host ? sample_plane_units(n * per_frame, W) : 0;
      const uint64_t units = P * pc.plane_units + (landed ? (n * OC + 7) & ~(uint64_t)7 : 0);
      staged.push_back(units);
      total += units;
      largest = std::max(largest, units);
    }
  }
  if (total) out->capacity = std::max(std::min(total, limit), largest) + 8;
  uint64_t used = 0;
  size_t batch = 0;
  for (size_t k = 0; k < out->pieces.size(); k++) {
    FormatPiece &pc = out->pieces[k];
    const FormatWindow &w = windows[pc.window];
    if (used && used + staged[k] > out->capacity) {
      batch++;
      used = 0;
    }
    pc.batch = batch;
    pc.raw_off = used;
    pc.mono_off = used + sample_format_planes(w.format, w.channels) * pc.plane_units;
    used += staged[k];
  }
  out->batches = out->pieces.empty() ? 0 : batch + 1;
  return Status::Ok();
}

// Host PCM with a format per stream -> kept items (fingerprint_host.hip), as gpu_fingerprint_host_format /
// gpu_fingerprint_streamed_device_format do for one format: the streams are uploaded raw and, launch group by launch
// group under the uploads that follow, landed as mono with ONE launch (`any_mix`: the rematrix kernel), resampled with one
// launch per distinct rate other than 11025 Hz, and fingerprinted.  `dst` of the streams is not looked at.  Items go to
// the host (`items`) or stay on the device (d_items_out + (*item_off_out)[i]).
Status gpu_fingerprint_formats(const std::vector<FormatWindow> &streams, bool any_mix, uint32_t step,
                               std::vector<std::vector<uint32_t>> *items, uint32_t *d_items_out = nullptr,
                               const std::vector<uint64_t> *item_off_out = nullptr);
// Same with the PCM produced by `read` as in gpu_fingerprint_streamed: every stream is interleaved s16 of its own channel
// count and rate (`src` is not looked at), read by up to `readers` threads into the ring of pinned slabs.
Status gpu_fingerprint_formats_streamed(const std::vector<FormatWindow> &streams, bool any_mix, const PcmReader &read, unsigned readers,
                                        uint32_t step, std::vector<std::vector<uint32_t>> *items);

}  // namespace needle
