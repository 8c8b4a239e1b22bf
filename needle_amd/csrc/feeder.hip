// Streaming fingerprinter (include/needle_hip.h needle_hip_feeder_*): N lanes, one per decoder; a feed takes what every
// lane has decoded since the last one, the per-lane state stays in HBM, and the items are bit for bit those of the
// one-shot path over the concatenation of a lane's chunks.
//
// State of a lane, bounded whatever the stream's length (two sets of buffers, see below):
//   * source-rate samples (converted, 3-8 channels down-mixed) the next resampler tile still reads -- other rates than
//     11025 Hz only;
//   * the 11025 Hz PCM tail, from the first frame of the first item not yet emitted (rounded down to a multiple of 4);
//   * the first pass's chroma and energy rows of the tail's whole frame pairs;
//   * audited (set_audit): the f64 kernel's chroma rows of the same frames, and six resident words of counts.
//
// One round (a feed, or a piece of one that exceeds the staging bound):
//   carry      feeder_carry_kernel: tails and rows of all lanes from the previous set of buffers to the front of their
//              places in the other set -- source and destination never alias, 16-byte accesses (a lane's place starts
//              at the same offset modulo 16 bytes as the data it inherits)
//   land       the new chunks behind the carried tails: copied straight (s16, 1-2 channels), or staged raw and
//              converted / down-mixed by convert.hip / downmix.hip; resample.hip then computes the whole output tiles
//              whose taps lie inside the samples fed (nothing is clamped before `finish` tells the stream's end).
//              A feeder whose lanes have formats of their own (CreateLanes) lands every lane as MONO instead: s16 mono
//              chunks copied straight, all others staged raw and reduced by one feeder_ingest_kernel launch whatever
//              the mixture (convert.hip); the resampler then runs once per distinct rate among the lanes that
//              complete tiles.  Stereo loses nothing by it: every reader of a stereo tail starts with the same
//              integer (L + R) / 2.  Lanes of such a feeder may have a channel mix (SetLaneMix); while any has one, the
//              staged chunks of a round land through one rematrix_kernel launch instead (rematrix.hip), the lanes
//              without a mix by the same ingest_block.
//   fingerprint gpu_fingerprint_feed_device (fingerprint.hip): the first pass over the NEW frame pairs only, behind the
//              carried rows; certification, recomputation and fix-up over carried + new.  Frame pairs are the
//              one-shot's (2p, 2p + 1): the tail starts at an even frame and a trailing odd frame waits for its partner
//              (or for `finish`, which transforms it alone as the one-shot does).
//   audit      only if asked for (set_audit), two more launches there: the f64 kernel over the new pairs into the audit's
//              own rows, audit_items_kernel over carried + new; the counts stay on the device until `audit` asks.
// Every step is one launch over all lanes (tables searched by block, as in downmix.hip / convert.hip).
//
// A lane's stream may change format on the way (SwitchFormat): it is then a sequence of SEGMENTS, each landed and
// resampled as a whole stream of its own, and the fingerprinter sees their 11025 Hz signals laid end to end as one
// stream.  Lane::seg_base is where the open segment starts in that signal; fed, tiles_done, src_p0, keep_p0 and src_off
// are the open segment's; a round adds seg_base to `samples` and to the resampler's out_off and is otherwise the round
// above.  A switch of lanes whose open segment resamples and holds samples is one round without chunks in which those
// lanes' last tiles are computed with the segment's end known (Chunk::flush: final_outputs as for `finish`, the frames
// kept even as for a feed); then the lane's source tail is dropped and the next segment begins at sample 0 of its own.
#include "feeder.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>

#include "hipctx.h"

namespace needle {

namespace {

constexpr uint32_t kLatency = (uint32_t)kItemLatency;  // frames - raw items

// ---- the carry ------------------------------------------------------------------------------------------------------
struct CarrySeg {
  const uint4 *src;
  uint4 *dst;
  uint32_t n16;         // 16-byte words
  uint32_t block_base;  // prefix of ceil(n16 / kCarryWordsPerBlock)
};
constexpr uint32_t kCarryThreads = 256, kCarryWordsPerThread = 4, kCarryWordsPerBlock = kCarryThreads * kCarryWordsPerThread;

__global__ __launch_bounds__(kCarryThreads) void feeder_carry_kernel(const CarrySeg *__restrict__ segs, int num_segs,
                                                                     uint32_t total_blocks) {
  const uint32_t b = blockIdx.x;
  if (b >= total_blocks) return;
  int lo = 0, hi = num_segs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].block_base <= b) lo = mid; else hi = mid - 1;
  }
  const CarrySeg sg = segs[lo];
  const uint32_t w0 = (b - sg.block_base) * kCarryWordsPerBlock + threadIdx.x;
  uint4 v[kCarryWordsPerThread];
#pragma unroll
  for (uint32_t k = 0; k < kCarryWordsPerThread; k++) {
    const uint32_t w = w0 + k * kCarryThreads;
    v[k] = w < sg.n16 ? sg.src[w] : make_uint4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (uint32_t k = 0; k < kCarryWordsPerThread; k++) {
    const uint32_t w = w0 + k * kCarryThreads;
    if (w < sg.n16) sg.dst[w] = v[k];
  }
}

struct BufferSet {
  DeviceBuffer<int16_t> src;     // source-rate tails + new samples (other rates than 11025 Hz)
  DeviceBuffer<int16_t> pcm;     // 11025 Hz tails + new samples, lane after lane
  DeviceBuffer<double> chroma;   // first-pass rows
  DeviceBuffer<float> energy;
  DeviceBuffer<double> audit64;  // the audit's f64 rows, numbered like chroma (empty unless audited)
};

struct Lane {
  uint64_t fed = 0;          // samples per channel fed (at the source rate) -- of the open segment, as tiles_done, src_p0,
                             // keep_p0 and src_off below are (a stream that never switched format is one segment)
  uint64_t samples = 0;      // 11025 Hz samples per channel the tail reaches to
  bool finished = false;
  uint64_t frames_done = 0;  // frames through the first pass (even unless finished)
  uint64_t items_done = 0;   // kept items emitted
  uint64_t tail_frame = 0;   // the frame the lane's place in the current set starts at
  uint64_t keep_frame = 0;   // ... and the one its place in the next set will start at (a multiple of 4, <= items_done * step)
  uint64_t pcm_off = 0;      // current set, s16 values
  uint32_t row_base = 0;     // current set
  // other rates than 11025 Hz: the resampler's output tiles computed, and the source samples kept for the next one
  uint64_t tiles_done = 0;
  uint64_t src_p0 = 0;       // the source sample the lane's place in the current set starts at
  uint64_t keep_p0 = 0;      // ... and the one its place in the next set will start at (resample_piece of the next tile)
  uint64_t src_off = 0;      // current set, s16 values
  // SwitchFormat: the 11025 Hz sample of the lane's stream the open segment starts at, and the segments ended before it
  uint64_t seg_base = 0;
  uint64_t fed_ended = 0;    // the sum of their frames
  std::vector<NeedleHipSegment> ended;
  std::vector<uint32_t> items;
  // of its current stream, in any segment: what SetAudit and SetLaneMix ask (`fed` alone is zero again after a switch,
  // while the lane still carries a tail and rows)
  bool holds_samples() const { return fed_ended + fed != 0; }
};

// 11025 Hz samples of a stream's first `fed` source samples that are final: every tap inside the samples fed (output m
// reads source samples up to m M / L + half), in whole tiles of the resampler -- or, finished, all of them.
uint64_t final_outputs(const ResampleTiling &t, uint64_t fed, bool finished, uint64_t *tiles) {
  const uint64_t L = (uint64_t)t.L, M = (uint64_t)t.M, half = (uint64_t)t.half;
  if (finished) {
    const uint64_t n_out = (fed * L + M - 1) / M;  // resample_out_len
    *tiles = (n_out + t.tile_outputs - 1) / t.tile_outputs;
    return n_out;
  }
  const uint64_t avail = fed > half ? ((fed - half) * L + M - 1) / M : 0;
  *tiles = avail / t.tile_outputs;
  return *tiles * t.tile_outputs;
}

}  // namespace

size_t feeder_num_ready_segments(const NeedleHipSegment *segments, size_t count, uint32_t step, bool finished) {
  if (!segments || !count || step == 0) return 0;
  uint64_t have = 0;  // 11025 Hz samples that are final
  for (size_t i = 0; i < count; i++) {
    const NeedleHipLaneFormat &f = segments[i].format;
    if (f.channels < 1 || f.channels > NEEDLE_HIP_MAX_CHANNELS || f.sample_rate < 2000 || f.sample_rate > 768000 || !sample_format_valid(f.format))
      return 0;
    const uint64_t n = segments[i].frames;
    if (i + 1 < count || finished || f.sample_rate == kSampleRate) {  // an ended segment is a whole stream of its own
      have += resample_out_len((size_t)n, f.sample_rate);
      continue;
    }
    ResampleTiling t;
    if (!resample_tiling_host(f.sample_rate, &t).ok()) return 0;
    uint64_t tiles = 0;
    have += final_outputs(t, n, false, &tiles);
  }
  if (finished) return num_kept((size_t)have, step);
  const uint64_t frames = (uint64_t)num_frames((size_t)have) & ~(uint64_t)1;
  const uint64_t raw = frames > kLatency ? frames - kLatency : 0;
  return (size_t)((raw + step - 1) / step);
}

size_t feeder_num_ready(uint64_t n, int sample_rate, int channels, uint32_t step, bool finished) {
  const NeedleHipSegment whole{NeedleHipLaneFormat{channels, sample_rate, NEEDLE_HIP_SAMPLE_S16}, n};  // (it has no sample format)
  return feeder_num_ready_segments(&whole, 1, step, finished);
}

struct Feeder::Impl {
  size_t n = 0;
  uint32_t step = 1;
  bool mixed = false;    // made by CreateLanes: a format per lane, every lane mono behind the landing
  int pcm_channels = 1;  // of the 11025 Hz tails: 3-8 channels arrive there down-mixed, resampled streams as mono
  int src_channels = 1;  // of what lands: 3-8 channels are down-mixed on the way
  // What a lane's stream is made of.  Create fills every lane alike; pcm_channels and src_channels are the feeder's in
  // both kinds (1 when mixed), since the chain behind the landing runs once over all lanes.
  struct Format {
    int channels = 1, rate = kSampleRate, format = NEEDLE_HIP_SAMPLE_S16;
    bool resample = false;
    const ResampleTiling *tiling = nullptr;  // the rate's, in `tilings`
    bool direct = true;  // chunks are copied straight behind the tails: s16 of 1-2 channels (mixed: s16 mono)
    size_t planes = 1, width = 2;
    size_t first_plane = 0;  // the lane's first pointer in feed's array
    bool has_mix = false;    // SetLaneMix: the lane is folded by `mix` as it lands (never direct then)
    NeedleHipChannelMix mix{};
  };
  std::vector<Format> fmt;
  std::map<int, ResampleTiling> tilings;  // of the distinct rates other than 11025 Hz, as counted when the lanes were made
  std::vector<Lane> lanes;
  BufferSet sets[2];
  int cur = 0;
  DeviceBuffer<double> chroma64;  // the recomputation's rows (fingerprint.hip)
  DeviceBuffer<int16_t> raw;      // chunks in the caller's format, as uploaded
  DeviceBuffer<uint32_t> d_items;
  DeviceBuffer<CarrySeg> d_segs;
  PinnedStage seg_stage, item_stage;
  hipEvent_t landed = nullptr;
  struct Pending { size_t lane; uint64_t off, count; };
  std::vector<Pending> pending;  // items on their way into item_stage
  Status poison = Status::Ok();
  uint64_t staging_high = 0;
  uint64_t state_high = 0;  // the most bytes a round carried for one lane (tails and rows)
  bool audit = false;
  DeviceBuffer<uint64_t> audit_counts;  // [n][kFeedAuditWords], zero where a lane's stream starts

  ~Impl() {
    std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
    if (landed) {
      (void)hipStreamSynchronize(library_stream());
      (void)hipEventDestroy(landed);
    }
    seg_stage.release();
    item_stage.release();
  }

  // the items of the last round: wait for them and append them to their lanes
  Status drain() {
    if (pending.empty()) return Status::Ok();
    NEEDLE_HIP_TRY(hipStreamSynchronize(library_stream()));
    item_stage.pending = false;
    const uint32_t *host = static_cast<const uint32_t *>(item_stage.ptr);
    for (const Pending &p : pending) lanes[p.lane].items.insert(lanes[p.lane].items.end(), host + p.off, host + p.off + p.count);
    pending.clear();
    return Status::Ok();
  }

  struct Chunk {
    const void *plane[NEEDLE_HIP_MAX_CHANNELS] = {};
    uint64_t frames = 0;  // samples per channel
    bool finish = false;
    bool flush = false;  // SwitchFormat: the open segment ends here (its last tiles are clamped), the lane's stream does not
  };

  // What a lane of the format (its limits checked by the caller) is made of, whole or not at all: a rate the resampler
  // has no design for fails here, before anything of the feeder has changed but, perhaps, an entry of `tilings` that no
  // lane uses (use_formats drops those).  first_plane is set by use_formats.
  Status make_format(const NeedleHipLaneFormat &lf, Format *out) {
    Format f;
    f.channels = lf.channels;
    f.rate = lf.sample_rate;
    f.format = lf.format;
    f.resample = lf.sample_rate != kSampleRate;
    if (f.resample) {
      auto it = tilings.find(f.rate);
      if (it == tilings.end()) {
        ResampleTiling t;
        Status s = resample_tiling_host(f.rate, &t);
        if (!s.ok()) return s;
        it = tilings.emplace(f.rate, t).first;
      }
      f.tiling = &it->second;
    }
    f.direct = mixed ? f.format % 5 == NEEDLE_HIP_SAMPLE_S16 && f.channels == 1 : f.format == NEEDLE_HIP_SAMPLE_S16 && f.channels <= 2;
    f.planes = sample_format_planes(f.format, f.channels);
    f.width = sample_format_width(f.format);
    *out = f;
    return Status::Ok();
  }
  // after `fmt` has changed: every lane's place in feed's pointer array, and no tiling of a rate no lane has
  void use_formats() {
    size_t at = 0;
    for (Format &f : fmt) {
      f.first_plane = at;
      at += f.planes;
    }
    for (auto it = tilings.begin(); it != tilings.end();) {
      bool used = false;
      for (const Format &f : fmt) used = used || f.tiling == &it->second;
      it = used ? std::next(it) : tilings.erase(it);
    }
  }

  Status round(const std::vector<Chunk> &chunks) {
    if (audit && gpu_fingerprint_f64_mode())
      return Status::Make(NeedleError_InvalidArgument, "feeder: NEEDLE_HIP_STFT=f64 has no first pass to audit");
    std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
    Status s = ensure_device();
    if (!s.ok()) return s;
    if (!(s = drain()).ok()) return s;
    hipStream_t stream = library_stream();
    if (!landed) NEEDLE_HIP_TRY(hipEventCreateWithFlags(&landed, hipEventDisableTiming));
    for (const auto &known : tilings) {  // the tiles a stream is counted in are the ones gpu_resample_device will plan
      ResampleTiling now;
      if (!(s = resample_tiling_host(known.first, &now)).ok()) return s;
      if (now.tile_outputs != known.second.tile_outputs) return Status::Make(NeedleError_Unknown, "feeder: the resampler's tiling changed under a stream");
    }
    BufferSet &from = sets[cur], &to = sets[cur ^ 1];
    struct Plan {
      uint64_t new_off = 0, carried_values = 0, src_off = 0, raw_off = 0;
      uint64_t new_src_off = 0, carried_src = 0, from_src_off = 0, tiles = 0, samples = 0;
      uint32_t row_base = 0, carried_rows = 0, src_row = 0;
      uint64_t frames = 0, kept = 0;  // after the round
    };
    std::vector<Plan> plan(n);
    std::vector<FeedLane> feed;
    std::vector<size_t> feed_lane;
    uint64_t cursor = 0, rows = 0, raw_units = 0, new_items = 0, new_values = 0, src_cursor = 0;
    bool any_resample = false;
    for (size_t i = 0; i < n; i++) {
      const Lane &l = lanes[i];
      const Chunk &c = chunks[i];
      const Format &f = fmt[i];
      any_resample = any_resample || f.resample;
      if (l.finished) continue;
      Plan &p = plan[i];
      p.carried_values = (l.samples - l.keep_frame * kHop) * (uint64_t)pcm_channels;
      p.src_off = l.pcm_off + (l.keep_frame - l.tail_frame) * kHop * (uint64_t)pcm_channels;
      p.carried_rows = (uint32_t)(l.frames_done - l.keep_frame);
      p.src_row = l.row_base + (uint32_t)(l.keep_frame - l.tail_frame);
      // the lane's place starts where its inherited data does modulo 16 bytes: the carry moves whole 16-byte words
      p.new_off = ((cursor + 7) & ~(uint64_t)7) + (p.carried_values ? p.src_off % 8 : 0);
      uint64_t samples = l.samples + c.frames;
      if (f.resample) {
        samples = l.seg_base + final_outputs(*f.tiling, l.fed + c.frames, c.finish || c.flush, &p.tiles);
        p.carried_src = (l.fed - l.keep_p0) * (uint64_t)src_channels;
        p.from_src_off = l.src_off + (l.keep_p0 - l.src_p0) * (uint64_t)src_channels;  // a multiple of 8 values: no skew
        p.new_src_off = (src_cursor + 7) & ~(uint64_t)7;
        src_cursor = p.new_src_off + (l.fed + c.frames - l.keep_p0) * (uint64_t)src_channels + 8;
      }
      p.samples = samples;
      cursor = p.new_off + samples * (uint64_t)pcm_channels - l.keep_frame * kHop * (uint64_t)pcm_channels + 8;
      new_values += c.frames * (uint64_t)src_channels;
      const uint64_t all = num_frames((size_t)samples);
      p.frames = c.finish ? all : all & ~(uint64_t)1;
      const uint64_t raw_items = p.frames > kLatency ? p.frames - kLatency : 0;
      p.kept = (raw_items + step - 1) / step;
      if (p.frames - l.keep_frame > 0x7FFFFFF0ull || rows > 0x7FFFFFF0ull) return Status::Make(NeedleError_InvalidArgument, "feeder: feed too large");
      p.row_base = (uint32_t)rows;
      rows += ((p.frames - l.keep_frame) + 3) & ~(uint64_t)1;
      if (!f.direct && c.frames) {
        p.raw_off = raw_units;
        raw_units += f.planes * sample_plane_units(c.frames * (f.planes == 1 ? (uint64_t)f.channels : 1), f.width);
      }
      if (p.frames > l.frames_done) {
        FeedLane fl{};
        fl.pcm_off = p.new_off;
        fl.item_off = new_items;
        fl.row_base = p.row_base;
        fl.carried = p.carried_rows;
        fl.frames = (uint32_t)(p.frames - l.keep_frame);
        fl.first_item = (uint32_t)(l.items_done * step - l.keep_frame);
        fl.kept = (uint32_t)(p.kept - l.items_done);
        fl.lane = (uint32_t)i;
        new_items += fl.kept;
        feed.push_back(fl);
        feed_lane.push_back(i);
      }
    }
    if (any_resample && !(s = to.src.reserve(src_cursor + 16)).ok()) return s;
    if (!(s = to.pcm.reserve(cursor + 16)).ok() || !(s = to.chroma.reserve((rows + 2) * kBands)).ok() ||
        !(s = to.energy.reserve((rows + 2) * 4)).ok() || !(s = chroma64.reserve((rows + 2) * kBands)).ok() ||
        !(s = d_items.reserve(std::max<uint64_t>(new_items, 1))).ok() || !(s = raw.reserve(std::max<uint64_t>(raw_units, 1))).ok())
      return s;
    if (audit && !(s = to.audit64.reserve((rows + 2) * kBands)).ok()) return s;
    staging_high = std::max(staging_high, (new_values + raw_units) * 2);

    // carry: tails and rows into the other set
    std::vector<CarrySeg> segs;
    uint32_t blocks = 0;
    auto add_seg = [&](const void *src, void *dst, uint64_t bytes) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(src), head = a & 15;
      CarrySeg sg;
      sg.src = reinterpret_cast<const uint4 *>(a - head);
      sg.dst = reinterpret_cast<uint4 *>(reinterpret_cast<uintptr_t>(dst) - head);
      sg.n16 = (uint32_t)((head + bytes + 15) / 16);
      sg.block_base = blocks;
      blocks += (sg.n16 + kCarryWordsPerBlock - 1) / kCarryWordsPerBlock;
      segs.push_back(sg);
    };
    for (size_t i = 0; i < n; i++) {
      const Lane &l = lanes[i];
      const Plan &p = plan[i];
      if (l.finished) continue;
      state_high = std::max(state_high, (p.carried_values + p.carried_src) * sizeof(int16_t) +
                                            (uint64_t)p.carried_rows * ((audit ? 2 : 1) * kBands * sizeof(double) + 4 * sizeof(float)));
      if (p.carried_values) add_seg(from.pcm.ptr + p.src_off, to.pcm.ptr + p.new_off, p.carried_values * 2);
      if (p.carried_src) add_seg(from.src.ptr + p.from_src_off, to.src.ptr + p.new_src_off, p.carried_src * 2);
      if (p.carried_rows) {
        add_seg(from.chroma.ptr + (uint64_t)p.src_row * kBands, to.chroma.ptr + (uint64_t)p.row_base * kBands,
                (uint64_t)p.carried_rows * kBands * sizeof(double));
        add_seg(from.energy.ptr + (uint64_t)p.src_row * 4, to.energy.ptr + (uint64_t)p.row_base * 4, (uint64_t)p.carried_rows * 4 * sizeof(float));
        if (audit)
          add_seg(from.audit64.ptr + (uint64_t)p.src_row * kBands, to.audit64.ptr + (uint64_t)p.row_base * kBands,
                  (uint64_t)p.carried_rows * kBands * sizeof(double));
      }
    }
    if (!segs.empty()) {
      if (!(s = d_segs.reserve(segs.size())).ok() || !(s = seg_stage.acquire(segs.size() * sizeof(CarrySeg))).ok()) return s;
      std::memcpy(seg_stage.ptr, segs.data(), segs.size() * sizeof(CarrySeg));
      NEEDLE_HIP_TRY(hipMemcpyAsync(d_segs.ptr, seg_stage.ptr, segs.size() * sizeof(CarrySeg), hipMemcpyHostToDevice, stream));
      seg_stage.mark(stream);
      KernelTimer timer("feeder_carry");
      hipLaunchKernelGGL(feeder_carry_kernel, dim3(blocks), dim3(kCarryThreads), 0, stream, d_segs.ptr, (int)segs.size(), blocks);
      NEEDLE_HIP_TRY(hipGetLastError());
    }

    // land: the new chunks behind the carried tails.  The caller's buffers are theirs again when this returns, so no
    // return, an error's included, leaves a copy reading them.
    struct CopiesDone {
      hipStream_t stream;
      bool waited = false;
      ~CopiesDone() { if (!waited) (void)hipStreamSynchronize(stream); }
    } copies{stream};
    std::vector<ConvertSpan> cspans;
    std::vector<DownmixSpan> mspans;
    std::vector<IngestSpan> ispans;
    bool any_mix = false;  // a lane of the feeder has a channel mix: every staged span lands through rematrix.hip
    for (const Format &f : fmt) any_mix = any_mix || f.has_mix;
    for (size_t i = 0; i < n; i++) {
      const Chunk &c = chunks[i];
      const Plan &p = plan[i];
      const Format &f = fmt[i];
      if (lanes[i].finished || !c.frames) continue;
      int16_t *dst = f.resample ? to.src.ptr + p.new_src_off + p.carried_src : to.pcm.ptr + p.new_off + p.carried_values;
      if (f.direct) {
        NEEDLE_HIP_TRY(hipMemcpyAsync(dst, c.plane[0], c.frames * (uint64_t)f.channels * 2, hipMemcpyHostToDevice, stream));
        continue;
      }
      const uint64_t plane_samples = c.frames * (f.planes == 1 ? (uint64_t)f.channels : 1), plane_units = sample_plane_units(plane_samples, f.width);
      ConvertSpan sp{};
      for (size_t k = 0; k < f.planes; k++) {
        int16_t *at = raw.ptr + p.raw_off + k * plane_units;
        NEEDLE_HIP_TRY(hipMemcpyAsync(at, c.plane[k], plane_samples * f.width, hipMemcpyHostToDevice, stream));
        sp.src[k] = at;
      }
      sp.dst = dst;
      sp.frames = c.frames;
      if (mixed) {
        IngestSpan in{};
        std::memcpy(in.src, sp.src, sizeof(in.src));
        in.dst = dst;
        in.frames = c.frames;
        in.channels = f.channels;
        in.format = f.format;
        in.mix = f.has_mix ? &f.mix : nullptr;
        ispans.push_back(in);
      } else if (f.format == NEEDLE_HIP_SAMPLE_S16) {
        mspans.push_back(DownmixSpan{raw.ptr + p.raw_off, dst, c.frames});
      } else {
        cspans.push_back(sp);
      }
    }
    NEEDLE_HIP_TRY(hipEventRecord(landed, stream));  // the caller's buffers are free once this has executed
    // (cspans and mspans: Create's feeder, every lane in the format of lane 0)
    if (!cspans.empty() && !(s = gpu_convert_device(cspans, fmt[0].channels, fmt[0].format, fmt[0].channels > 2, false)).ok()) return s;
    if (!mspans.empty() && !(s = gpu_downmix_device(mspans, fmt[0].channels, false)).ok()) return s;
    if (!ispans.empty() && !(s = any_mix ? gpu_rematrix_device(ispans, false) : gpu_ingest_device(ispans, false)).ok()) return s;
    // the whole tiles whose taps lie inside the samples fed, behind the 11025 Hz tails: the resampler's plan and tile
    // shape belong to a rate, so one launch per distinct rate among the lanes that complete tiles
    for (const auto &known : tilings) {
      std::vector<ResampleSpan> rspans;
      for (size_t i = 0; i < n; i++) {
        const Lane &l = lanes[i];
        const Plan &p = plan[i];
        if (fmt[i].rate != known.first || l.finished || p.tiles <= l.tiles_done) continue;
        ResampleSpan sp{};
        sp.n_in = l.fed + chunks[i].frames;
        sp.out_off = p.new_off - l.keep_frame * kHop + l.seg_base;  // of the segment's output 0 (modulo 2^64, common.h)
        sp.src = to.src.ptr + p.new_src_off;
        sp.t0 = l.tiles_done;
        sp.t1 = p.tiles;
        sp.p0 = l.keep_p0;
        sp.p1 = sp.n_in;
        rspans.push_back(sp);
      }
      if (!rspans.empty() && !(s = gpu_resample_device(nullptr, rspans, src_channels, known.first, to.pcm.ptr, false)).ok()) return s;
    }

    if (!feed.empty()) {
      const FeedAudit audited{to.audit64.ptr, audit_counts.ptr};
      if (!(s = gpu_fingerprint_feed_device(to.pcm.ptr, feed, pcm_channels, step, to.chroma.ptr, to.energy.ptr, chroma64.ptr, d_items.ptr,
                                            audit ? &audited : nullptr)).ok())
        return s;
      if (new_items) {
        if (!(s = item_stage.acquire(new_items * sizeof(uint32_t))).ok()) return s;
        NEEDLE_HIP_TRY(hipMemcpyAsync(item_stage.ptr, d_items.ptr, new_items * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        item_stage.mark(stream);
        for (size_t k = 0; k < feed.size(); k++)
          if (feed[k].kept) pending.push_back(Pending{feed_lane[k], feed[k].item_off, feed[k].kept});
      }
    }
    for (size_t i = 0; i < n; i++) {
      Lane &l = lanes[i];
      const Plan &p = plan[i];
      if (l.finished) continue;
      l.fed += chunks[i].frames;
      l.samples = p.samples;
      if (fmt[i].resample) {
        const ResampleTiling &tiling = *fmt[i].tiling;
        l.src_p0 = l.keep_p0;
        l.src_off = p.new_src_off;
        l.tiles_done = p.tiles;
        // what the next tile reads from (resample_piece)
        const long long first = (long long)(l.tiles_done * tiling.tile_outputs * (uint64_t)tiling.M / (uint64_t)tiling.L) - tiling.half + 1;
        l.keep_p0 = std::max(l.keep_p0, std::min<uint64_t>(first <= 0 ? 0 : (uint64_t)first & ~(uint64_t)7, l.fed & ~(uint64_t)7));
      }
      l.tail_frame = l.keep_frame;
      l.pcm_off = p.new_off;
      l.row_base = p.row_base;
      l.frames_done = p.frames;
      l.items_done = p.kept;
      // (a multiple of 4 frames: a lane's two-pair chunks are then the groups of four frames the one-shot lists)
      l.keep_frame = std::max(l.keep_frame, std::min(l.items_done * step, l.frames_done) & ~(uint64_t)3);
      if (chunks[i].finish) l.finished = true;
    }
    cur ^= 1;
    NEEDLE_HIP_TRY(hipEventSynchronize(landed));
    copies.waited = true;
    return Status::Ok();
  }

  Status guarded_round(const std::vector<Chunk> &chunks) {
    Status s = round(chunks);
    if (!s.ok() && s.code != NeedleError_InvalidArgument && s.code != NeedleError_NullArgument) poison = s;
    return s;
  }
};

Feeder::Feeder() : impl_(new Impl()) {}
Feeder::~Feeder() = default;
size_t Feeder::lanes() const { return impl_->n; }
uint32_t Feeder::step() const { return impl_->step; }

namespace {

Status check_lane_format(const NeedleHipLaneFormat &f) {
  if (f.channels < 1 || f.channels > NEEDLE_HIP_MAX_CHANNELS)
    return Status::Make(NeedleError_InvalidArgument, "feeder: channels must be 1 to " + std::to_string(NEEDLE_HIP_MAX_CHANNELS));
  if (f.sample_rate < 2000 || f.sample_rate > 768000) return Status::Make(NeedleError_InvalidArgument, "feeder: unsupported sample rate");
  if (!sample_format_valid(f.format)) return Status::Make(NeedleError_InvalidArgument, "feeder: unknown sample format");
  return Status::Ok();
}

}  // namespace

Status Feeder::Create(size_t lanes, int channels, int sample_rate, int format, uint32_t step, std::unique_ptr<Feeder> *out) {
  if (lanes == 0 || lanes > (1u << 20)) return Status::Make(NeedleError_InvalidArgument, "feeder: lanes must be 1 to 1048576");
  const NeedleHipLaneFormat all{channels, sample_rate, format};
  Status s = check_lane_format(all);
  if (!s.ok()) return s;
  if (step == 0) return Status::Make(NeedleError_InvalidArgument, "feeder: step must be >= 1");
  std::unique_ptr<Feeder> f(new Feeder());
  Impl &m = *f->impl_;
  m.n = lanes;
  m.step = step;
  m.src_channels = channels > 2 ? 1 : channels;
  m.pcm_channels = sample_rate != kSampleRate ? 1 : m.src_channels;
  Impl::Format made;
  if (!(s = m.make_format(all, &made)).ok()) return s;
  m.fmt.assign(lanes, made);
  m.use_formats();
  m.lanes.resize(lanes);
  *out = std::move(f);
  return Status::Ok();
}

Status Feeder::CreateLanes(const NeedleHipLaneFormat *formats, size_t lanes, uint32_t step, std::unique_ptr<Feeder> *out) {
  if (!formats || !out) return Status::Make(NeedleError_NullArgument, "feeder: null argument");
  if (lanes == 0 || lanes > (1u << 20)) return Status::Make(NeedleError_InvalidArgument, "feeder: lanes must be 1 to 1048576");
  Status s;
  for (size_t i = 0; i < lanes; i++)
    if (!(s = check_lane_format(formats[i])).ok()) return s;
  if (step == 0) return Status::Make(NeedleError_InvalidArgument, "feeder: step must be >= 1");
  std::unique_ptr<Feeder> f(new Feeder());
  Impl &m = *f->impl_;
  m.n = lanes;
  m.step = step;
  m.mixed = true;  // src_channels = pcm_channels = 1
  m.fmt.resize(lanes);
  for (size_t i = 0; i < lanes; i++)
    if (!(s = m.make_format(formats[i], &m.fmt[i])).ok()) return s;
  m.use_formats();
  m.lanes.resize(lanes);
  *out = std::move(f);
  return Status::Ok();
}

Status Feeder::LaneFormat(size_t lane, NeedleHipLaneFormat *format) const {
  if (!format) return Status::Make(NeedleError_NullArgument, "feeder: null argument");
  if (lane >= impl_->n) return Status::Make(NeedleError_InvalidArgument, "feeder: lane out of range");
  const Impl::Format &f = impl_->fmt[lane];
  *format = NeedleHipLaneFormat{f.channels, f.rate, f.format};
  return Status::Ok();
}

Status Feeder::ResetFormat(const size_t *lanes, const NeedleHipLaneFormat *formats, size_t k) {
  Impl &m = *impl_;
  if (!lanes || !formats) return Status::Make(NeedleError_NullArgument, "feeder: null argument");
  if (!m.mixed) return Status::Make(NeedleError_InvalidArgument, "feeder: one format for all lanes (needle_hip_feeder_new): a lane cannot change it");
  Status s = Status::Ok();
  for (size_t j = 0; j < k; j++) {
    if (lanes[j] >= m.n) return Status::Make(NeedleError_InvalidArgument, "feeder: lane out of range");
    if (!(s = check_lane_format(formats[j])).ok()) return s;
  }
  // every new format whole (a rate without a resampler design fails here) before any lane is reset or changed
  std::vector<Impl::Format> made(k);
  for (size_t j = 0; j < k && s.ok(); j++) s = m.make_format(formats[j], &made[j]);
  if (s.ok()) s = Reset(lanes, k);
  if (s.ok())
    for (size_t j = 0; j < k; j++) m.fmt[lanes[j]] = made[j];
  m.use_formats();
  return s;
}

Status Feeder::SwitchFormat(const size_t *lanes, const NeedleHipLaneFormat *formats, const NeedleHipChannelMix *mixes, size_t k) {
  Impl &m = *impl_;
  if (!lanes || !formats) return Status::Make(NeedleError_NullArgument, "feeder: null argument");
  if (!m.mixed) return Status::Make(NeedleError_InvalidArgument, "feeder: one format for all lanes (needle_hip_feeder_new): a lane cannot change it");
  if (!m.poison.ok()) return m.poison;
  Status s = Status::Ok();
  std::vector<bool> named(m.n, false);
  for (size_t j = 0; j < k; j++) {  // every lane, every format and every mix before any lane changes
    if (lanes[j] >= m.n) return Status::Make(NeedleError_InvalidArgument, "feeder: lane out of range");
    if (named[lanes[j]]) return Status::Make(NeedleError_InvalidArgument, "feeder: a lane named twice in one switch");
    named[lanes[j]] = true;
    if (!(s = check_lane_format(formats[j])).ok()) return s;
    if (mixes && mixes[j].channels && !(s = channel_mix_check(mixes[j], formats[j].channels)).ok()) return s;
    if (m.lanes[lanes[j]].finished) return Status::Make(NeedleError_InvalidArgument, "feeder: the lane is finished (reset it first)");
  }
  std::vector<Impl::Format> made(k);
  for (size_t j = 0; j < k && s.ok(); j++) s = m.make_format(formats[j], &made[j]);
  if (!s.ok()) {
    m.use_formats();  // (drops a tiling make_format added for a lane named before the refused one)
    return s;
  }
  // the flush round: the open segments that resample end as whole streams do, all lanes of the call in one round
  std::vector<Impl::Chunk> chunks(m.n);
  bool any = false;
  for (size_t j = 0; j < k; j++)
    if (m.fmt[lanes[j]].resample && m.lanes[lanes[j]].fed) chunks[lanes[j]].flush = any = true;
  if (any && !(s = m.guarded_round(chunks)).ok()) {
    m.use_formats();
    return s;
  }
  for (size_t j = 0; j < k; j++) {
    Lane &l = m.lanes[lanes[j]];
    Impl::Format &f = m.fmt[lanes[j]];
    l.ended.push_back(NeedleHipSegment{NeedleHipLaneFormat{f.channels, f.rate, f.format}, l.fed});
    l.fed_ended += l.fed;
    l.seg_base = l.samples;
    l.fed = l.tiles_done = l.src_p0 = l.keep_p0 = l.src_off = 0;  // the source tail is dropped: every output that read it exists
    f = made[j];
    f.has_mix = mixes && mixes[j].channels != 0;
    if (f.has_mix) {
      f.mix = mixes[j];
      f.direct = false;
    }
  }
  m.use_formats();
  return Status::Ok();
}

Status Feeder::LaneSegments(size_t lane, NeedleHipSegment *out, size_t cap, size_t *count) const {
  const Impl &m = *impl_;
  if (!count || (cap && !out)) return Status::Make(NeedleError_NullArgument, "feeder: null argument");
  if (lane >= m.n) return Status::Make(NeedleError_InvalidArgument, "feeder: lane out of range");
  const Lane &l = m.lanes[lane];
  const Impl::Format &f = m.fmt[lane];
  *count = l.ended.size() + 1;
  for (size_t i = 0; i < std::min(cap, l.ended.size()); i++) out[i] = l.ended[i];
  if (cap > l.ended.size()) out[l.ended.size()] = NeedleHipSegment{NeedleHipLaneFormat{f.channels, f.rate, f.format}, l.fed};
  return Status::Ok();
}

Status Feeder::SetLaneMix(const size_t *lanes, const NeedleHipChannelMix *mixes, size_t k) {
  Impl &m = *impl_;
  if (!lanes || !mixes) return Status::Make(NeedleError_NullArgument, "feeder: null argument");
  if (!m.mixed) return Status::Make(NeedleError_InvalidArgument, "feeder: one format for all lanes (needle_hip_feeder_new): a lane cannot have a channel mix");
  if (!m.poison.ok()) return m.poison;
  Status s;
  for (size_t j = 0; j < k; j++) {  // every lane and every mix before any lane changes
    if (lanes[j] >= m.n) return Status::Make(NeedleError_InvalidArgument, "feeder: lane out of range");
    const Lane &l = m.lanes[lanes[j]];
    if (l.holds_samples() || l.finished) return Status::Make(NeedleError_InvalidArgument, "feeder: a lane's channel mix is set only while it holds no samples");
    if (mixes[j].channels && !(s = channel_mix_check(mixes[j], m.fmt[lanes[j]].channels)).ok()) return s;
  }
  for (size_t j = 0; j < k; j++) {
    Impl::Format &f = m.fmt[lanes[j]];
    f.has_mix = mixes[j].channels != 0;
    f.mix = f.has_mix ? mixes[j] : NeedleHipChannelMix{};
    f.direct = !f.has_mix && f.format % 5 == NEEDLE_HIP_SAMPLE_S16 && f.channels == 1;  // (make_format's rule of such a feeder)
  }
  return Status::Ok();
}

Status Feeder::Feed(const void *const *pcm, const size_t *num_values) {
  Impl &m = *impl_;
  if (!pcm || !num_values) return Status::Make(NeedleError_NullArgument, "feeder: null argument");
  if (!m.poison.ok()) return m.poison;
  bool any = false;
  for (size_t i = 0; i < m.n; i++) {
    const Impl::Format &f = m.fmt[i];
    if (num_values[i] % (size_t)f.channels) return Status::Make(NeedleError_InvalidArgument, "feeder: a chunk must be whole frames");
    if (!num_values[i]) continue;
    if (m.lanes[i].finished) return Status::Make(NeedleError_InvalidArgument, "feeder: the lane is finished (reset it first)");
    for (size_t k = 0; k < f.planes; k++)
      if (!pcm[f.first_plane + k]) return Status::Make(NeedleError_NullArgument, "feeder: null chunk");
    any = true;
  }
  if (!any) return Status::Ok();
  // a feed beyond the staging bound is cut into rounds (the bound counts values, as in the one-shot entry points)
  uint64_t bound = 1ull << 30;
  if (const char *e = getenv("NEEDLE_HIP_MAX_BATCH_VALUES")) bound = (uint64_t)std::max(1ll, atoll(e));
  std::vector<uint64_t> done(m.n, 0);
  for (;;) {
    std::vector<Impl::Chunk> chunks(m.n);
    uint64_t left = bound;  // values
    bool more = false, took = false;
    for (size_t i = 0; i < m.n; i++) {
      const Impl::Format &f = m.fmt[i];
      const uint64_t frames = num_values[i] / (size_t)f.channels;
      // (a round moves at least one frame, however small the bound)
      const uint64_t fit = std::max<uint64_t>(left / (uint64_t)f.channels, took ? 0 : 1), take = std::min(frames - done[i], fit);
      if (take) {
        const uint64_t first = done[i] * (f.planes == 1 ? (uint64_t)f.channels : 1) * f.width;  // bytes into every plane
        for (size_t k = 0; k < f.planes; k++) chunks[i].plane[k] = static_cast<const char *>(pcm[f.first_plane + k]) + first;
        chunks[i].frames = take;
        done[i] += take;
        left -= std::min(left, take * (uint64_t)f.channels);
        took = true;
      }
      more = more || done[i] < frames;
    }
    Status s = m.guarded_round(chunks);
    if (!s.ok() || !more) return s;
  }
}

Status Feeder::Finish(const size_t *lanes, size_t k) {
  Impl &m = *impl_;
  if (!m.poison.ok()) return m.poison;
  std::vector<Impl::Chunk> chunks(m.n);
  bool any = false;
  for (size_t j = 0; j < (lanes ? k : m.n); j++) {
    const size_t i = lanes ? lanes[j] : j;
    if (i >= m.n) return Status::Make(NeedleError_InvalidArgument, "feeder: lane out of range");
    if (m.lanes[i].finished) continue;
    chunks[i].finish = true;
    any = true;
  }
  return any ? m.guarded_round(chunks) : Status::Ok();
}

Status Feeder::Reset(const size_t *lanes, size_t k) {
  Impl &m = *impl_;
  if (!m.poison.ok()) return m.poison;
  for (size_t j = 0; j < (lanes ? k : m.n); j++)
    if (lanes && lanes[j] >= m.n) return Status::Make(NeedleError_InvalidArgument, "feeder: lane out of range");
  if (!m.pending.empty()) {
    std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
    Status s = m.drain();
    if (!s.ok()) return m.poison = s;
  }
  if (m.audit) {  // a lane's audit is its current stream's (behind the rounds that still count into it: one stream)
    std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
    for (size_t j = 0; j < (lanes ? k : m.n); j++) {
      const hipError_t e = hipMemsetAsync(m.audit_counts.ptr + (lanes ? lanes[j] : j) * kFeedAuditWords, 0,
                                          kFeedAuditWords * sizeof(uint64_t), library_stream());
      if (e != hipSuccess) return m.poison = Status::Make(NeedleError_Unknown, std::string("HIP error: ") + hipGetErrorString(e));
    }
  }
  for (size_t j = 0; j < (lanes ? k : m.n); j++) m.lanes[lanes ? lanes[j] : j] = Lane();
  return Status::Ok();
}

Status Feeder::SetAudit(bool on) {
  Impl &m = *impl_;
  if (!m.poison.ok()) return m.poison;
  for (const Lane &l : m.lanes)
    if (l.holds_samples() || l.finished) return Status::Make(NeedleError_InvalidArgument, "feeder: the audit is switched only while no lane holds samples");
  if (on && gpu_fingerprint_f64_mode())
    return Status::Make(NeedleError_InvalidArgument, "feeder: NEEDLE_HIP_STFT=f64 has no first pass to audit");
  if (on) {
    std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
    Status s = ensure_device();
    if (!s.ok() || !(s = m.audit_counts.reserve(m.n * kFeedAuditWords)).ok()) return s;
    NEEDLE_HIP_TRY(hipMemsetAsync(m.audit_counts.ptr, 0, m.n * kFeedAuditWords * sizeof(uint64_t), library_stream()));
  }
  m.audit = on;
  return Status::Ok();
}

Status Feeder::Audit(size_t lane, uint64_t counts[4], double *max_ratio, double *max_sigma) {
  Impl &m = *impl_;
  if (!m.audit) return Status::Make(NeedleError_InvalidArgument, "feeder: the audit is off (set_audit)");
  if (lane >= m.n && lane != SIZE_MAX) return Status::Make(NeedleError_InvalidArgument, "feeder: lane out of range");
  if (!m.poison.ok()) return m.poison;
  const size_t first = lane == SIZE_MAX ? 0 : lane, count = lane == SIZE_MAX ? m.n : 1;
  std::vector<uint64_t> host(count * kFeedAuditWords);
  {
    std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
    hipStream_t stream = library_stream();
    NEEDLE_HIP_TRY(hipMemcpyAsync(host.data(), m.audit_counts.ptr + first * kFeedAuditWords, host.size() * sizeof(uint64_t),
                                  hipMemcpyDeviceToHost, stream));
    NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  }
  uint64_t bits[2] = {0, 0};  // doubles >= 0 compare like their bit patterns
  for (int c = 0; c < 4; c++) counts[c] = 0;
  for (size_t i = 0; i < count; i++) {
    for (int c = 0; c < 4; c++) counts[c] += host[i * kFeedAuditWords + c];
    for (int c = 0; c < 2; c++) bits[c] = std::max(bits[c], host[i * kFeedAuditWords + 4 + c]);
  }
  std::memcpy(max_ratio, &bits[0], sizeof(double));
  std::memcpy(max_sigma, &bits[1], sizeof(double));
  return Status::Ok();
}

Status Feeder::Ready(size_t lane, size_t *kept_items, uint64_t *samples_fed, bool *finished) {
  Impl &m = *impl_;
  if (lane >= m.n) return Status::Make(NeedleError_InvalidArgument, "feeder: lane out of range");
  if (!m.poison.ok()) return m.poison;
  if (!m.pending.empty()) {
    std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
    Status s = m.drain();
    if (!s.ok()) return m.poison = s;
  }
  if (kept_items) *kept_items = m.lanes[lane].items.size();
  if (samples_fed) *samples_fed = m.lanes[lane].fed_ended + m.lanes[lane].fed;
  if (finished) *finished = m.lanes[lane].finished;
  return Status::Ok();
}

Status Feeder::Items(size_t lane, size_t first, size_t count, uint32_t *items) {
  size_t have = 0;
  Status s = Ready(lane, &have, nullptr, nullptr);
  if (!s.ok()) return s;
  if (first > have || count > have - first) return Status::Make(NeedleError_InvalidArgument, "feeder: items out of range");
  if (count && !items) return Status::Make(NeedleError_NullArgument, "feeder: null argument");
  if (count) std::memcpy(items, impl_->lanes[lane].items.data() + first, count * sizeof(uint32_t));
  return Status::Ok();
}

Status Feeder::FinishedItems(size_t lane, const std::vector<uint32_t> **items) {
  bool finished = false;
  Status s = Ready(lane, nullptr, nullptr, &finished);
  if (!s.ok()) return s;
  if (!finished) return Status::Make(NeedleError_InvalidArgument, "feeder: the lane is not finished");
  *items = &impl_->lanes[lane].items;
  return Status::Ok();
}

void Feeder::StateBytes(uint64_t bytes[2]) const {
  bytes[0] = impl_->state_high;
  bytes[1] = impl_->staging_high;
}

}  // namespace needle
