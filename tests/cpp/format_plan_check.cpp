// The host plan of a library's PCM on its way in (needle_amd/csrc/format_plan.h), under ASan/UBSan: the walk over the
// pointer array with planar and NULL videos, and the cut of every window into pieces and batches, per rate, from the
// host and from the device, whole and with staging limits that force many pieces and one tile per piece -- for a season
// with a format per video and for uniform libraries of every landing kind.  Every source plane and the staging buffer
// are allocated at exactly their size and the uploads and landings are replayed with memcpy / memset, so a piece that
// reads past its plane or lands past the staging is an ASan report.  Host code only, no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "format_plan.h"

using namespace needle;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

static const NeedleHipLaneFormat kSeason[7] = {
    {1, 11025, NEEDLE_HIP_SAMPLE_S16}, {2, 11025, NEEDLE_HIP_SAMPLE_S16}, {2, 44100, NEEDLE_HIP_SAMPLE_S16},
    {6, 48000, NEEDLE_HIP_SAMPLE_F32P}, {2, 48000, NEEDLE_HIP_SAMPLE_S32}, {1, 32000, NEEDLE_HIP_SAMPLE_U8P},
    {2, 22050, NEEDLE_HIP_SAMPLE_F64}};

static void check_walk() {
  const std::vector<size_t> first = format_first_planes(kSeason, 7);
  const size_t want[8] = {0, 1, 2, 3, 9, 10, 11, 12};
  for (size_t v = 0; v <= 7; v++) CHECK(first[v] == want[v]);
  int x = 0;
  std::vector<const void *> pcm(12, &x);
  std::vector<char> held;
  CHECK(format_walk_planes(pcm.data(), first, &held).ok());
  for (size_t v = 0; v < 7; v++) CHECK(held[v]);
  for (size_t p = 3; p < 9; p++) pcm[p] = nullptr;  // the planar video lives on another rank
  pcm[0] = nullptr;
  CHECK(format_walk_planes(pcm.data(), first, &held).ok());
  CHECK(!held[0] && held[1] && held[2] && !held[3] && held[4] && held[5] && held[6]);
  pcm[5] = &x;  // one plane of six
  CHECK(format_walk_planes(pcm.data(), first, &held).code == NeedleError_NullArgument);
  pcm[5] = nullptr;
  pcm[3] = &x;  // the first plane alone
  CHECK(format_walk_planes(pcm.data(), first, &held).code == NeedleError_NullArgument);
}

// The uniform libraries of library.cpp's format_windows, one per landing kind: what the resampler reads is the raw
// stereo (no landing), the down-mixed or rematrixed mono, or the converted 1-2 channels; two land at 11025 Hz.
struct Uniform {
  NeedleHipLaneFormat format;
  Landing landing;
  int out_channels;
};
static const Uniform kUniform[7] = {
    {{2, 48000, NEEDLE_HIP_SAMPLE_S16}, Landing::None, 2},     {{6, 11025, NEEDLE_HIP_SAMPLE_S16}, Landing::Downmix, 1},
    {{6, 48000, NEEDLE_HIP_SAMPLE_S16}, Landing::Downmix, 1},  {{2, 44100, NEEDLE_HIP_SAMPLE_F32}, Landing::Convert, 2},
    {{2, 11025, NEEDLE_HIP_SAMPLE_S32}, Landing::Convert, 2},  {{6, 48000, NEEDLE_HIP_SAMPLE_F32P}, Landing::Convert, 1},
    {{2, 32000, NEEDLE_HIP_SAMPLE_S16}, Landing::Rematrix, 1}};

// `uniform`: nullptr for the season of seven formats (every window ingested as mono), or one of kUniform for all videos
static void check_plan(const Uniform *uniform, bool from_host, uint64_t limit, bool count_values, size_t *pieces_out,
                       size_t *mixed_batches_out) {
  std::map<int, ResampleTiling> tilings;
  std::vector<FormatWindow> windows;
  std::vector<std::vector<uint8_t *>> planes;
  // an opening and an ending window per video, of odd lengths; one video has none (another rank's)
  for (size_t v = 0; v < 7; v++) {
    const NeedleHipLaneFormat &f = uniform ? uniform->format : kSeason[v];
    if (f.sample_rate != kSampleRate) CHECK(resample_tiling_host(f.sample_rate, &tilings[f.sample_rate]).ok());
    if (v == 4) continue;
    for (int r = 0; r < 2; r++) {
      FormatWindow w;
      w.frames = (uint64_t)f.sample_rate * (r ? 3 : 7) + 13 * v + r;
      w.channels = f.channels;
      w.format = f.format;
      w.rate = f.sample_rate;
      if (uniform) {
        w.landing = uniform->landing;
        w.out_channels = uniform->out_channels;
      }
      const size_t P = sample_format_planes(f.format, f.channels);
      const size_t bytes = w.frames * (P == 1 ? f.channels : 1) * sample_format_width(f.format);
      planes.emplace_back();
      for (size_t c = 0; c < P; c++) {
        planes.back().push_back(static_cast<uint8_t *>(std::malloc(bytes)));  // exactly the plane
        std::memset(planes.back().back(), (int)(v + c), bytes);
        w.src[c] = planes.back().back();
      }
      windows.push_back(w);
    }
  }
  windows.push_back(FormatWindow{});  // a window without frames
  FormatPlan plan;
  CHECK(format_plan_pieces(windows, tilings, from_host, limit, count_values, &plan).ok());
  CHECK(!plan.pieces.empty() && plan.batches >= 1);
  if (uniform && uniform->landing == Landing::None && !from_host) {  // resampled out of the caller's buffers: nothing staged,
    CHECK(plan.capacity == 0 && plan.batches == 1 && plan.pieces.size() == 12);  // one piece of all its tiles per window
    for (const FormatPiece &pc : plan.pieces) CHECK(pc.t0 == 0 && pc.p0 == 0 && pc.p1 == windows[pc.window].frames);
  }
  int16_t *stage = plan.capacity ? static_cast<int16_t *>(std::malloc(plan.capacity * sizeof(int16_t))) : nullptr;
  std::vector<uint64_t> next_frame(windows.size(), 0), next_tile(windows.size(), 0);
  size_t batch = 0, mixed_batches = 0;
  uint64_t used = 0;
  long batch_format = -1;  // (channels, rate, format) of the batch's first piece; -2 once another one has joined it
  for (const FormatPiece &pc : plan.pieces) {
    const FormatWindow &w = windows[pc.window];
    const uint64_t n = pc.p1 - pc.p0, W = sample_format_width(w.format);
    const size_t P = sample_format_planes(w.format, w.channels);
    const uint64_t per_frame = P == 1 ? (uint64_t)w.channels : 1;
    CHECK(n > 0 && pc.p1 <= w.frames);
    CHECK(pc.batch == batch || pc.batch == batch + 1);
    if (pc.batch != batch) {
      batch = pc.batch;
      used = 0;
      batch_format = -1;
    }
    const long video_format = ((long)w.rate * 16 + w.channels) * 16 + w.format;
    if (batch_format == -1) {
      batch_format = video_format;
    } else if (batch_format >= 0 && batch_format != video_format) {
      batch_format = -2;
      mixed_batches++;
    }
    CHECK(pc.raw_off == used);  // pieces of a batch lie one behind the other
    CHECK(pc.raw_off % 8 == 0 && pc.plane_units % 8 == 0 && pc.mono_off % 8 == 0);
    if (w.rate == kSampleRate) {
      CHECK(pc.p0 == next_frame[pc.window] && pc.p0 % 16 == 0);  // whole 16-frame groups, in order, no gaps
      next_frame[pc.window] = pc.p1;
    } else {
      const ResampleTiling &tl = tilings[w.rate];
      uint64_t p0 = 0, p1 = 0;
      CHECK(pc.t0 == next_tile[pc.window] && pc.t1 > pc.t0);  // whole tiles of the rate's own tiling, in order
      resample_piece(tl, w.frames, pc.t0, pc.t1, &p0, &p1);
      CHECK(p0 == pc.p0 && p1 == pc.p1 && pc.p0 % 8 == 0);
      next_tile[pc.window] = pc.t1;
    }
    for (size_t c = 0; c < P; c++) {
      const uint8_t *from = static_cast<const uint8_t *>(w.src[c]) + pc.p0 * per_frame * W;
      if (from_host) {
        CHECK(pc.plane_units * 2 >= n * per_frame * W);
        std::memcpy(stage + pc.raw_off + c * pc.plane_units, from, n * per_frame * W);  // the upload
      } else {
        volatile uint8_t first = from[0], last = from[n * per_frame * W - 1];  // read in place
        (void)first;
        (void)last;
      }
    }
    // the raw region [raw_off, mono_off) and the landed one behind it: disjoint, inside the capacity, and the next
    // piece of the batch begins where they end (CHECK(pc.raw_off == used) above)
    CHECK(pc.mono_off == pc.raw_off + P * pc.plane_units);
    used = pc.mono_off;
    if (w.rate != kSampleRate && w.landing != Landing::None) {
      const uint64_t values = n * (uint64_t)w.out_channels;
      std::memset(stage + pc.mono_off, 0, values * sizeof(int16_t));  // what the landing kernel writes
      used += (values + 7) & ~(uint64_t)7;
    } else if (w.rate != kSampleRate && from_host) {
      CHECK(P == 1 && W == 2 && pc.plane_units >= n * (uint64_t)w.out_channels);  // the resampler reads the raw staging
    }
    CHECK(used <= plan.capacity);
  }
  CHECK(batch + 1 == plan.batches);
  for (size_t i = 0; i < windows.size(); i++) {
    const FormatWindow &w = windows[i];
    if (w.rate == kSampleRate) {
      CHECK(next_frame[i] == w.frames);
    } else {
      const ResampleTiling &tl = tilings[w.rate];
      CHECK(next_tile[i] == (resample_out_len(w.frames, w.rate) + tl.tile_outputs - 1) / tl.tile_outputs);
    }
  }
  if (!from_host && limit >= 1ull << 30) CHECK(plan.batches == 1);
  *pieces_out = plan.pieces.size();
  *mixed_batches_out = mixed_batches;
  std::free(stage);
  for (auto &v : planes)
    for (uint8_t *p : v) std::free(p);
}

int main() {
  check_walk();
  size_t whole = 0, medium = 0, small = 0, tile = 0, mixed = 0;
  for (int from_host = 0; from_host < 2; from_host++) {
    check_plan(nullptr, from_host, 1ull << 30, false, &whole, &mixed);
    CHECK(whole == 12 && mixed == 1);  // one piece per window, one batch of every format
    check_plan(nullptr, from_host, 400003, true, &medium, &mixed);
    std::printf("from_host %d, 400003 values: %zu pieces, %zu batches of more than one format\n", from_host, medium, mixed);
    CHECK(mixed >= 1);  // batches that hold pieces of different formats
    check_plan(nullptr, from_host, 3001, true, &small, &mixed);
    std::printf("from_host %d, 3001 values: %zu pieces, %zu batches of more than one format\n", from_host, small, mixed);
    CHECK(mixed >= 1);
    check_plan(nullptr, from_host, 1, true, &tile, &mixed);
    CHECK(tile >= small && small > medium && medium > whole);
    for (const Uniform &u : kUniform) {
      const bool staged = from_host || (u.landing != Landing::None && u.format.sample_rate != kSampleRate);
      check_plan(&u, from_host, 1ull << 30, false, &whole, &mixed);
      CHECK(whole == 12 && mixed == 0);
      check_plan(&u, from_host, 400003, false, &medium, &mixed);  // the limit in bytes, as without the variable
      check_plan(&u, from_host, 3001, true, &small, &mixed);
      check_plan(&u, from_host, 1, true, &tile, &mixed);
      if (staged) CHECK(tile >= small && small >= medium && medium > whole);  // (one tile per piece may be reached early)
      else CHECK(tile == whole && small == whole && medium == whole);  // read in place: the limit cuts nothing
    }
  }
  // a rate the resampler has no tiling for is refused, not planned
  FormatWindow w;
  w.frames = 1000;
  w.rate = 48000;
  int16_t x[1000] = {};
  w.src[0] = x;
  FormatPlan plan;
  CHECK(format_plan_pieces({w}, {}, true, 1ull << 30, false, &plan).code == NeedleError_InvalidArgument);
  std::puts("format plan ok");
  return 0;
}
