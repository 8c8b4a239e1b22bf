// NeedleHipLibrary: an HBM-resident analyze+search job (include/needle_hip.h, last section).
//
// The reference's library path is Analyzer::run -> Comparator::run_with_frame_hashes
// (needle/src/audio/analyzer.rs:425, comparator.rs:524): analyze every video, then search every pair.
// Here the PCM of the videos a rank owns stays in HBM, hashes are written straight into a padded device
// arena u32[rows][stride] (one row per video and search window: row v*R = opening, v*R+1 = ending when
// endings are enabled), the pair search reads that arena in place, and only the short run list crosses
// PCIe — the runs carry their simhashes, so the host epilogue needs timestamps only.  Rows computed by
// other ranks are filled by the caller with one all-gather over contiguous row blocks (RCCL over xGMI);
// pairs are sharded by index in the lexicographic pair list -- or, in a library with groups of videos
// (needle_hip_library_set_groups), by grouped pair id (pair_ids.h): only pairs inside a group exist.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <tuple>

#include "comm.h"
#include "epilogue.h"
#include "format_plan.h"
#include "hipctx.h"
#include "job_plan.h"
#include "needle_core.h"
#include "pair_ids.h"

struct FrameHashes;
struct NeedleAudioComparator;

namespace needle {
const Comparator &comparator_of(const NeedleAudioComparator *c);
FrameHashes *make_frame_hashes(FrameHashesData &&d);
void fill_c_result(const VideoResult &v, NeedleHipSearchResult *r);
}  // namespace needle

using namespace needle;

namespace {
struct Window {              // one search window of one video
  size_t values = 0;         // interleaved s16 values
  uint64_t pcm_off = ~0ull;  // offset into d_pcm; ~0 when this rank does not hold the PCM
  uint32_t kept = 0;         // hashes kept (every step-th raw item)
  ns_t seek = 0;             // added to every timestamp (ending window, analyzer.rs:314-318)
};
}  // namespace

struct NeedleHipLibrary {
  size_t n = 0;
  float opening_pct = DEFAULT_OPENING_SEARCH_PERCENTAGE;
  float ending_pct = DEFAULT_ENDING_SEARCH_PERCENTAGE;
  bool endings = false;
  ns_t hash_duration = 0;
  uint32_t step = 0;
  int channels = 1;            // of the resident PCM (1 whenever it was down-mixed or resampled on the way in)
  int rate = kSampleRate;      // of the callers' PCM (needle_hip_library_set_sample_rate); the resident PCM is 11025 Hz
  int format = NEEDLE_HIP_SAMPLE_S16;  // of the callers' PCM (needle_hip_library_set_sample_format); the resident PCM is s16
  bool has_mix = false;                // needle_hip_library_set_channel_mix: the callers' PCM is folded to mono by `mix` on the way in
  NeedleHipChannelMix mix{};
  bool uniform_set = false;            // one of the three setters above was called: needle_hip_library_set_video_formats is refused
  // needle_hip_library_set_video_formats: a format and a mix (channels == 0: the plain average) per video.  Every video
  // lands as 11025 Hz mono s16; rate, format, mix and channels above are not looked at.
  bool has_formats = false;
  bool any_mix = false;
  std::vector<NeedleHipLaneFormat> formats;
  std::vector<NeedleHipChannelMix> mixes;
  // needle_hip_library_set_groups: a label per video; only pairs inside a group are searched, numbered as pair_ids.h
  // numbers them (GroupTables, built once).  Null: a plain library, all pairs in the i-major numbering.
  std::vector<uint32_t> group_labels;
  std::unique_ptr<const GroupTables> groups;
  std::vector<uint64_t> hash_durations;  // grouped: the device epilogue's one value per video (all the library's own)
  // the tables in device memory for the owner-directed exchange's kernel, uploaded once per library (ensure_device_groups)
  struct DeviceGroups {
    DeviceBuffer<uint32_t> group_of, rank_of, size, first, members;
    DeviceBuffer<uint64_t> base;
    bool uploaded = false;
    GroupView view{};
  } d_groups;
  size_t pairs() const { return groups ? (size_t)groups->pairs() : pair_count(n); }
  bool have_pcm = false;      // windows and arena are set up (set_pcm or stream_pcm)
  bool pcm_resident = false;  // set_pcm: the PCM stays in HBM and analyze can be repeated
  std::vector<Window> win;  // [video * regions() + region]
  size_t stride = 0;
  DeviceBuffer<int16_t> d_pcm;
  DeviceBuffer<uint32_t> d_arena;
  uint32_t *arena = nullptr;  // d_arena.ptr, or caller-owned memory adopted with needle_hip_library_use_hash_arena
  std::vector<std::vector<HashTs>> ts_cache;  // un-seeked timestamps by kept length
  std::vector<uint32_t> min_len;              // per row, for the durations below
  ns_t min_len_for[2] = {~0ull, ~0ull};
  // the pair table of the last search, reused while (first pair, pair count, regions, min_len) stay the same: a
  // library has ~n^2 / 2 pairs and a job that is repeated should not rebuild millions of descriptors
  std::vector<NeedleHipProblem> problems;
  size_t problems_for[3] = {~(size_t)0, 0, 0};
  // Timestamps for the epilogue (the hashes stay in HBM).  A window's timestamps are a function of its length and seek
  // only, so videos of equal geometry SHARE one shell: at library scale the epilogue's four timestamp reads per run
  // then hit one 87 KB array instead of 2000 copies of it (174 MB of cache misses: 58 -> 15 ms of the heap-entry phase).
  std::vector<FrameHashesData> shells;        // distinct geometries
  std::vector<uint32_t> shell_of;             // video -> shells[]
  // double-buffered asynchronous run-list download (needle_hip_library_fetch_runs_begin / _end)
  struct Fetch {
    void *host = nullptr;  // pinned: u32 count, then max_runs NeedleHipRun
    uint32_t max_runs = 0;
    hipEvent_t ready = nullptr, done = nullptr;  // search enqueued (library stream) / copies finished (download stream)
    const NeedleHipRun *d_runs = nullptr;        // what the pending download reads
    const uint32_t *d_count = nullptr;
    bool pending = false;
  } fetch[2];
  // One slot of the job pipeline (needle_hip_library_job_begin / _end).  Rank r's slab = 32-byte header (word 0: runs found) +
  // slab_runs runs (job_plan.h); the scan writes straight into this rank's slab, the other ranks' runs arrive as heads or
  // as the blocks of the owner-directed exchange.
  struct Job {
    bool pending = false;
    // What was planned when the job -- or its repeat -- was enqueued (job_plan.h plan_job), and what the enqueue made of it.
    struct Planned {
      JobPlan plan;
      bool device_epilogue = false;  // plan.device_epilogue, unless the device form failed on THIS rank at the enqueue
      bool counted = false;          // host_counts holds this job's count matrix
      bool directed = false;         // this job's runs travelled owner-directed (plan.directed.sized and a transport that can)
      uint32_t scan_form = 0;
    } planned;
    // What job_end found (needle_hip_library_job_runs / _form / _comm_bytes).
    struct Found {
      std::vector<NeedleHipRun> merged;
      const NeedleHipRun *last_runs = nullptr;  // the complete run list of the job that finished last in this slot
      size_t last_total = 0;
      std::vector<NeedleHipRun> fetched;  // directed: the received runs, downloaded on demand (job_runs, a host fallback)
      bool fetched_valid = false;
      bool ran_device_epilogue = false, ran_sharded = false;
      uint64_t comm_bytes[4] = {0, 0, 0, 0};  // received per rank in this job: hash rows, run heads, results; scans repeated
    } found;
    // Owner-directed run exchange (world > 1 with the sharded device epilogue): a run of pair (i, j) travels to the owners of
    // videos i and j only (comparator.rs:583-588: a video's epilogue needs its own pairs), not to every rank.  d_dir_send =
    // this rank's runs sorted into one block per destination (epilogue.h DirectPlan), d_dir_recv = the blocks received, in
    // rank order, = the device epilogue's segments; d_dir_counts = the count matrix (job_plan.h), all-gathered, host_counts
    // its download.  A count beyond its block is the head overflow's case (job_end: sizes grow, the job is repeated).
    struct Buffers {
      DeviceBuffer<uint8_t> d_slabs;  // this rank's slab only
      DeviceBuffer<uint8_t> d_heads;  // world > 1: [world][head_bytes], what the all-gather of run lists fills
      DeviceBuffer<uint8_t> d_dir_send, d_dir_recv;
      DeviceBuffer<uint32_t> d_dir_counts;
      uint32_t slab_runs = 0;  // what d_slabs was allocated for
      int world = 0;
      PinnedBuffer host;          // the heads of all ranks, in one copy
      PinnedBuffer host_counts;   // the count matrix
      PinnedBuffer host_results;  // device epilogue: per-video results + failure count land here behind the run download
      hipEvent_t searched = nullptr, done = nullptr;
    } buf;
  } job[2];
  JobHistory history;  // what the last finished job leaves the next one (job_plan.h): every rank holds the same
  size_t arena_rows = 0;       // rows the arena was allocated with
  const uint32_t *count_zeroed = nullptr;  // a run counter the last kernel of this job's analyze has just cleared (job_begin)
  // what the device epilogue needs to know about the arena's rows (built once per geometry: plan_windows clears them)
  std::vector<uint32_t> row_len, row_ts;
  std::vector<uint64_t> row_seek, ts_tables;
  void ensure_row_tables() {
    if (row_len.size() == rows()) return;
    row_len.assign(rows(), 0);
    row_ts.assign(rows(), 0);
    row_seek.assign(rows(), 0);
    ts_tables.clear();
    std::map<uint32_t, uint32_t> offset_of;  // kept length -> offset of its un-seeked timestamps
    for (size_t row = 0; row < rows(); row++) {
      const Window &w = win[row];
      auto it = offset_of.find(w.kept);
      if (it == offset_of.end()) {
        it = offset_of.emplace(w.kept, (uint32_t)ts_tables.size()).first;
        for (const HashTs &h : timestamps(w.kept)) ts_tables.push_back(h.ts);
      }
      row_len[row] = w.kept;
      row_ts[row] = it->second;
      row_seek[row] = w.seek;
    }
  }
  ~NeedleHipLibrary() {
    for (Fetch &f : fetch) {
      if (f.host) (void)hipHostFree(f.host);
      if (f.done) (void)hipEventDestroy(f.done);
      if (f.ready) (void)hipEventDestroy(f.ready);
    }
    for (Job &j : job) {
      if (j.buf.done) (void)hipEventDestroy(j.buf.done);
      if (j.buf.searched) (void)hipEventDestroy(j.buf.searched);
    }
  }

  size_t regions() const { return endings ? 2 : 1; }
  size_t rows() const { return n * regions(); }
  // Sharding of the fingerprinting across ranks (analyzer.rs:437-445 across GPUs).  The unit is not the video but the
  // HASH: the arena u32[rows][stride] is cut, as one flat array, into world equal blocks -- stride is a multiple of 64
  // chosen so that rows * stride divides by 64 * world -- and a rank fingerprints exactly the hashes of its block:
  // for every row the block meets, the columns it meets, computed from the SUB-WINDOW of that row's PCM those hashes
  // depend on (hash k of a row is a function of frames k * step .. k * step + 19 only; blocks start on multiples of 64
  // hashes, so a sub-window starts on an even frame and the two-frames-per-transform pairing is the whole window's).
  // 28 episodes on 8 ranks are then 3.5 rows each instead of 7 x 4 + 0; one in-place all-gather of equal blocks
  // fills the arena as before.
  size_t flat_block(int world) const { return rows() * stride / (size_t)std::max(world, 1); }
  bool flat_shardable(int world) const { return world <= 1 || (stride % 64 == 0 && (rows() * (stride / 64)) % (size_t)world == 0); }
  void ensure_shells() {
    if (shell_of.size() == n) return;
    shells.clear();
    shell_of.assign(n, 0);
    const size_t R = regions();
    std::map<std::tuple<uint32_t, ns_t, uint32_t, ns_t>, uint32_t> seen;
    for (size_t v = 0; v < n; v++) {
      const Window &wo = win[v * R];
      const Window we = endings ? win[v * R + 1] : Window{};
      const auto key = std::make_tuple(wo.kept, wo.seek, we.kept, we.seek);
      auto it = seen.find(key);
      if (it == seen.end()) {
        FrameHashesData d;
        d.opening = window_timestamps(wo);
        if (endings) d.ending = window_timestamps(we);
        d.hash_duration = hash_duration;
        it = seen.emplace(key, (uint32_t)shells.size()).first;
        shells.push_back(std::move(d));
      }
      shell_of[v] = it->second;
    }
  }
  std::vector<const FrameHashesData *> shell_pointers() {
    ensure_shells();
    std::vector<const FrameHashesData *> fh(n);
    for (size_t v = 0; v < n; v++) fh[v] = &shells[shell_of[v]];
    return fh;
  }

  const std::vector<HashTs> &timestamps(uint32_t k) {
    if (ts_cache.size() <= k) ts_cache.resize(k + 1);
    if (ts_cache[k].empty() && k) {
      std::vector<uint32_t> zeros(k, 0);
      attach_timestamps(zeros.data(), k, step, false, 0, &ts_cache[k]);
    }
    return ts_cache[k];
  }
  std::vector<HashTs> window_timestamps(const Window &w) {
    std::vector<HashTs> ts = timestamps(w.kept);
    if (w.seek)
      for (HashTs &h : ts) h.ts += w.seek;
    return ts;
  }
};

namespace {
template <typename F>
NeedleError guarded(F &&f) {
  try {
    return f();
  } catch (const std::bad_alloc &) {
    return report(Status::Make(NeedleError_Unknown, "out of memory"));
  } catch (...) {
    return report(Status::Make(NeedleError_Unknown, "internal error"));
  }
}
}  // namespace

extern "C" {

enum NeedleError needle_hip_library_new(size_t num_videos, float opening_search_percentage, float hash_duration,
                                        NeedleHipLibrary **output) {
  if (!output) return NeedleError_NullArgument;
  if (num_videos == 0) return NeedleError_InvalidArgument;
  if (!(hash_duration > 0.0f)) return NeedleError_AnalyzerInvalidHashDuration;
  return guarded([&]() -> NeedleError {
    bool ok = true;
    const ns_t hd = duration_from_secs_f32(hash_duration, &ok);
    uint32_t step = 0;
    if (!ok || !step_for_hash_duration(hd, &step)) return NeedleError_AnalyzerInvalidHashDuration;
    auto *lib = new NeedleHipLibrary();
    lib->n = num_videos;
    lib->opening_pct = opening_search_percentage;
    lib->hash_duration = hd;
    lib->step = step;
    *output = lib;
    return NeedleError_Ok;
  });
}

void needle_hip_library_free(NeedleHipLibrary *library) { delete library; }

enum NeedleError needle_hip_library_include_endings(NeedleHipLibrary *lib, float ending_search_percentage) {
  if (!lib) return NeedleError_NullArgument;
  if (lib->have_pcm) return NeedleError_InvalidArgument;  // must precede set_pcm
  lib->endings = true;
  lib->ending_pct = ending_search_percentage;
  return NeedleError_Ok;
}

enum NeedleError needle_hip_library_set_sample_rate(NeedleHipLibrary *lib, int sample_rate) {
  if (!lib) return NeedleError_NullArgument;
  if (sample_rate < 2000 || sample_rate > 768000) return NeedleError_InvalidArgument;  // Analyzer::run_pcm's range
  if (lib->have_pcm || lib->has_formats) return NeedleError_InvalidArgument;  // must precede set_pcm; not beside set_video_formats
  ResampleTiling tiling;  // a rate the resampler has no kernel for is refused here, not at the first set_pcm
  if (sample_rate != kSampleRate) {
    Status s = resample_tiling_host(sample_rate, &tiling);
    if (!s.ok()) return report(s);
  }
  lib->rate = sample_rate;
  lib->uniform_set = true;
  return NeedleError_Ok;
}

enum NeedleError needle_hip_library_set_sample_format(NeedleHipLibrary *lib, int format) {
  if (!lib) return NeedleError_NullArgument;
  if (!sample_format_valid(format)) return NeedleError_InvalidArgument;
  if (lib->have_pcm || lib->has_formats) return NeedleError_InvalidArgument;  // must precede set_pcm; not beside set_video_formats
  lib->format = format;
  lib->uniform_set = true;
  return NeedleError_Ok;
}

enum NeedleError needle_hip_library_set_channel_mix(NeedleHipLibrary *lib, const NeedleHipChannelMix *mix) {
  if (!lib) return NeedleError_NullArgument;
  if (lib->have_pcm || lib->has_formats) return NeedleError_InvalidArgument;  // must precede set_pcm; not beside set_video_formats
  if (mix) {
    Status s = channel_mix_check(*mix, mix->channels);
    if (!s.ok()) return report(s);
    lib->mix = *mix;
  }
  lib->has_mix = mix != nullptr;
  lib->uniform_set = true;
  return NeedleError_Ok;
}

enum NeedleError needle_hip_library_set_video_formats(NeedleHipLibrary *lib, const NeedleHipLaneFormat *formats,
                                                      const NeedleHipChannelMix *mixes) {
  if (!lib || !formats) return NeedleError_NullArgument;
  if (lib->have_pcm || lib->uniform_set) return NeedleError_InvalidArgument;  // before any PCM; not beside the three setters
  return guarded([&]() -> NeedleError {
    // every video is checked before anything changes, on the host
    bool any_mix = false;
    for (size_t v = 0; v < lib->n; v++) {
      const NeedleHipChannelMix *mix = mixes && mixes[v].channels ? &mixes[v] : nullptr;
      Status s = lane_format_check(formats[v], mix, "video " + std::to_string(v));
      if (!s.ok()) return report(s);
      any_mix = any_mix || mix;
    }
    std::vector<NeedleHipLaneFormat> fs(formats, formats + lib->n);
    std::vector<NeedleHipChannelMix> ms(lib->n, NeedleHipChannelMix{});
    if (mixes) ms.assign(mixes, mixes + lib->n);
    lib->formats.swap(fs);
    lib->mixes.swap(ms);
    lib->any_mix = any_mix;
    lib->has_formats = true;
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_library_video_format(const NeedleHipLibrary *lib, size_t video, NeedleHipLaneFormat *format) {
  if (!lib || !format) return NeedleError_NullArgument;
  if (!lib->has_formats || video >= lib->n) return NeedleError_InvalidArgument;
  *format = lib->formats[video];
  return NeedleError_Ok;
}

enum NeedleError needle_hip_library_set_groups(NeedleHipLibrary *lib, const uint32_t *groups, size_t num_videos) {
  if (!lib || !groups) return NeedleError_NullArgument;
  if (lib->have_pcm || num_videos != lib->n || num_videos > UINT32_MAX) return NeedleError_InvalidArgument;  // must precede set_pcm
  return guarded([&]() -> NeedleError {
    std::vector<uint32_t> labels(groups, groups + num_videos);
    std::unique_ptr<const GroupTables> tables(new GroupTables(groups, num_videos));
    std::vector<uint64_t> durations(num_videos, lib->hash_duration);
    lib->group_labels.swap(labels);
    lib->groups = std::move(tables);
    lib->hash_durations.swap(durations);
    lib->d_groups.uploaded = false;
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_library_groups(const NeedleHipLibrary *lib, uint32_t *labels, size_t n) {
  if (!lib || !labels) return NeedleError_NullArgument;
  if (!lib->groups || n < lib->n) return NeedleError_InvalidArgument;  // a plain library has none
  std::copy(lib->group_labels.begin(), lib->group_labels.end(), labels);
  return NeedleError_Ok;
}

}  // extern "C"

namespace {
// the channel count of a set_pcm / set_pcm_device / stream_pcm call against the library's mix, before any device is asked for
Status check_mix_channels(const NeedleHipLibrary *lib, int channels) {
  return lib->has_mix ? channel_mix_check(lib->mix, channels) : Status::Ok();
}

// Samples a window of `count` samples at `rate` keeps resident (11025 Hz).
size_t resident_samples(size_t count, int rate) { return rate == kSampleRate ? count : resample_out_len(count, rate); }

// What plan_windows and rank_videos read per video: the call's one format, or the video's own (set_video_formats).
struct VideoLayout {
  int channels, rate, format;
  size_t planes, width, first_plane;
};
struct VideoLayouts {
  const NeedleHipLibrary *lib;
  int channels;
  std::vector<size_t> first;  // formats: where each video's planes begin in the caller's pointer array
  VideoLayouts(const NeedleHipLibrary *l, int call_channels) : lib(l), channels(call_channels) {
    if (lib->has_formats) first = format_first_planes(lib->formats.data(), lib->n);
  }
  VideoLayout operator()(size_t v) const {
    if (lib->has_formats) {
      const NeedleHipLaneFormat &f = lib->formats[v];
      return VideoLayout{f.channels, f.sample_rate, f.format, first[v + 1] - first[v], sample_format_width(f.format), first[v]};
    }
    const size_t planes = sample_format_planes(lib->format, channels);
    return VideoLayout{channels, lib->rate, lib->format, planes, sample_format_width(lib->format), v * planes};
  }
};

// the `channels` of a PCM call or of rank_videos: 1..8 for a library with one format, 0 for one with a format per video
bool call_channels_ok(const NeedleHipLibrary *lib, int channels) {
  return lib->has_formats ? channels == 0 : channels >= 1 && channels <= NEEDLE_HIP_MAX_CHANNELS;
}

// A grouped library's tables in device memory (pair_ids.h GroupView), for the kernel that sorts the runs by destination:
// uploaded once per library, when its PCM is set (a few words per video; no job waits for it).
template <class T>
Status upload_table(DeviceBuffer<T> *dst, const std::vector<T> &src) {
  Status s = dst->reserve(std::max<size_t>(src.size(), 1));
  if (!s.ok()) return s;
  if (!src.empty()) NEEDLE_HIP_TRY(hipMemcpy(dst->ptr, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return Status::Ok();
}
Status ensure_device_groups(NeedleHipLibrary *lib) {
  NeedleHipLibrary::DeviceGroups &d = lib->d_groups;
  if (d.uploaded) return Status::Ok();
  const GroupTables &t = *lib->groups;
  Status s;
  if (!(s = upload_table(&d.group_of, t.group_of)).ok() || !(s = upload_table(&d.rank_of, t.rank_of)).ok() ||
      !(s = upload_table(&d.size, t.size)).ok() || !(s = upload_table(&d.first, t.first)).ok() ||
      !(s = upload_table(&d.members, t.members)).ok() || !(s = upload_table(&d.base, t.base)).ok())
    return s;
  d.view = GroupView{d.group_of.ptr, d.rank_of.ptr, d.size.ptr, d.first.ptr, d.base.ptr, d.members.ptr, (uint32_t)t.size.size()};
  d.uploaded = true;
  return Status::Ok();
}

// Search windows of every video (analyzer.rs:378,390) from the stream lengths, arena geometry, and -- for the videos
// whose PCM this rank holds -- where each window starts in the caller's buffer.  `resident`: the windows get offsets
// into the device PCM arena (set_pcm); otherwise nothing of the PCM is kept (stream_pcm).  `len` is in the caller's
// (interleaved) values at lib->rate; windows are cut at that rate (as Analyzer::run_pcm does).  3-8 channel PCM and PCM
// at any rate other than 11025 Hz are kept resident as 11025 Hz mono (down-mixed and resampled on the way in), so
// lib->channels and the windows' `values` describe the arena, not the input; `len` is the input's.  The samples are in
// lib->format: `pcm` holds one pointer per video, or -- planar -- one per channel of every video, and `src` gets as many
// per window (anything but interleaved s16 is converted on the way in, 3-8 channels to mono by the same kernel; with a
// channel mix everything goes that way and arrives as mono, rematrix.hip).
// With a format per video (set_video_formats; channels == 0) rate, channels, format and the number of planes are the
// video's own: `pcm` is the concatenation of every video's planes, every window is resident as 11025 Hz mono, `len` is in
// the video's own values and `video_of_src` says whose window each entry is.
Status plan_windows(NeedleHipLibrary *lib, const void *const *pcm, const size_t *num_values, int channels, bool resident,
                    std::vector<const void *> *src, std::vector<size_t> *len, std::vector<uint64_t> *dst,
                    std::vector<uint64_t> *rows_of_src, uint64_t *total_values, std::vector<size_t> *video_of_src = nullptr) {
  Status s = ensure_device();
  if (!s.ok()) return s;
  const bool resampled = lib->rate != kSampleRate, converted = lib->format != NEEDLE_HIP_SAMPLE_S16 || lib->has_mix;
  const VideoLayouts video(lib, channels);
  std::vector<size_t> first_planes(lib->n + 1);  // a video is held with all its planes or with none
  for (size_t v = 0; v <= lib->n; v++) first_planes[v] = v < lib->n ? video(v).first_plane : video(v - 1).first_plane + video(v - 1).planes;
  if (!(s = format_walk_planes(pcm, first_planes)).ok()) return s;
  lib->channels = lib->has_formats || channels > 2 || resampled || lib->has_mix ? 1 : channels;
  const size_t R = lib->regions();
  lib->win.assign(lib->rows(), Window{});
  uint64_t total = 0;
  uint32_t max_kept = 0;
  std::vector<size_t> first_sample(lib->rows(), 0), source_samples(lib->rows(), 0);
  for (size_t v = 0; v < lib->n; v++) {
    const VideoLayout l = video(v);
    const size_t samples = num_values[v] / (size_t)l.channels;
    size_t open_samples = 0, end_first = 0;
    ns_t seek = 0;
    s = Analyzer::windows(samples, l.rate, lib->opening_pct, lib->ending_pct, &open_samples, &end_first, &seek);
    if (!s.ok()) return s;
    for (size_t r = 0; r < R; r++) {
      Window &w = lib->win[v * R + r];
      const size_t count = r == 0 ? open_samples : samples - end_first;
      const size_t kept_samples = resident_samples(count, l.rate);
      first_sample[v * R + r] = r == 0 ? 0 : end_first;
      source_samples[v * R + r] = count;
      w.values = kept_samples * (size_t)lib->channels;
      w.kept = (uint32_t)num_kept(kept_samples, lib->step);
      w.seek = r == 0 ? 0 : seek;
      max_kept = std::max(max_kept, w.kept);
      if (pcm[l.first_plane] && resident) {
        w.pcm_off = total;
        total += lib->has_formats || channels > 2 || resampled || converted ? (w.values + 7) & ~(uint64_t)7 : (w.values + 1) & ~(uint64_t)1;  // (down-mix: 16-byte stores)
      }
    }
  }
  // rows start 256-byte aligned; with a communicator, rows * stride also divides into world blocks of whole 64-hash tiles
  size_t tiles_per_row = std::max<size_t>(1, ((size_t)max_kept + 63) / 64);
  while (comm_world() > 1 && (lib->rows() * tiles_per_row) % (size_t)comm_world()) tiles_per_row++;
  size_t stride = 64 * tiles_per_row;
  const size_t arena_rows = lib->rows();
  // NeedleHipSeq.offset and NeedleHipProblem.tag are 32-bit on the device
  if ((uint64_t)arena_rows * stride > UINT32_MAX || (uint64_t)lib->pairs() * R > UINT32_MAX)
    return Status::Make(NeedleError_InvalidArgument, "library too large for one job: more than 2^32 arena hashes or sequence pairs");
  const bool own_arena = lib->arena == lib->d_arena.ptr;
  if (!lib->arena || (own_arena && (stride != lib->stride || arena_rows != lib->arena_rows))) {
    if (!(s = lib->d_arena.reserve(arena_rows * stride)).ok()) return s;
    lib->arena = lib->d_arena.ptr;
    lib->arena_rows = arena_rows;
    lib->stride = stride;
    if (hipMemsetAsync(lib->arena, 0, arena_rows * stride * sizeof(uint32_t), library_stream()) != hipSuccess)
      return Status::Make(NeedleError_Unknown, "hipMemset failed");
  } else if (!own_arena && (stride > lib->stride || arena_rows > lib->arena_rows)) {
    return Status::Make(NeedleError_InvalidArgument, "the adopted hash arena is too small for these videos");
  }
  for (size_t v = 0; v < lib->n; v++) {
    const VideoLayout l = video(v);
    for (size_t r = 0; r < R; r++) {
      const Window &w = lib->win[v * R + r];
      if (!pcm[l.first_plane] || !w.values) continue;
      for (size_t c = 0; c < l.planes; c++)  // a plane holds one sample per frame, an interleaved stream `channels`
        src->push_back(static_cast<const uint8_t *>(pcm[l.first_plane + c]) +
                       first_sample[v * R + r] * (l.planes == 1 ? (size_t)l.channels : 1) * l.width);
      len->push_back(source_samples[v * R + r] * (size_t)l.channels);
      if (dst) dst->push_back(w.pcm_off);
      if (rows_of_src) rows_of_src->push_back(v * R + r);
      if (video_of_src) video_of_src->push_back(v);
    }
  }
  if (total_values) *total_values = total;
  if (lib->groups && !(s = ensure_device_groups(lib)).ok()) return s;
  lib->min_len.clear();
  lib->row_len.clear();
  lib->shells.clear();
  lib->shell_of.clear();
  lib->problems_for[0] = ~(size_t)0;
  return Status::Ok();
}

std::vector<const int16_t *> as_s16(const std::vector<const void *> &src) {
  std::vector<const int16_t *> out(src.size());
  for (size_t i = 0; i < src.size(); i++) out[i] = static_cast<const int16_t *>(src[i]);
  return out;
}

// The windows plan_windows lists, as the plan (format_plan.h) and the launches read them: window i belongs to video
// video_of[i] and `src` holds that video's planes for it.  Rate, channels, format and mix are the video's own
// (set_video_formats) or the library's, from its setters and the call's `channels`; so is the landing.  A uniform
// library keeps the kernel its route always had -- the conversion kernels run at 79-81 % of the copy rate, the ingest
// and rematrix kernels at 42-53 % -- and its 1-2 channels stay 1-2 channels behind it unless a mix folds them.
std::vector<FormatWindow> format_windows(const NeedleHipLibrary *lib, int channels, const std::vector<const void *> &src,
                                         const std::vector<size_t> &len, const std::vector<uint64_t> *dst,
                                         const std::vector<size_t> &video_of) {
  std::vector<FormatWindow> windows(len.size());
  size_t plane = 0;
  for (size_t i = 0; i < len.size(); i++) {
    const size_t v = video_of[i];
    const NeedleHipLaneFormat f = lib->has_formats ? lib->formats[v] : NeedleHipLaneFormat{channels, lib->rate, lib->format};
    FormatWindow &w = windows[i];
    for (size_t c = 0; c < sample_format_planes(f.format, f.channels); c++) w.src[c] = src[plane++];
    w.frames = len[i] / (uint64_t)f.channels;
    w.channels = f.channels;
    w.format = f.format;
    w.rate = f.sample_rate;
    w.dst = dst ? (*dst)[i] : 0;
    if (lib->has_formats) {
      w.mix = lib->mixes[v].channels ? &lib->mixes[v] : nullptr;
      w.landing = lib->any_mix ? Landing::Rematrix : Landing::Ingest;
    } else {
      w.mix = lib->has_mix ? &lib->mix : nullptr;
      w.landing = lib->has_mix                         ? Landing::Rematrix
                  : f.format != NEEDLE_HIP_SAMPLE_S16  ? Landing::Convert
                  : channels > 2                       ? Landing::Downmix
                                                       : Landing::None;
      w.out_channels = lib->has_mix || channels > 2 ? 1 : channels;
    }
  }
  return windows;
}

// One launch of landing kernel `kind` over the spans of a batch (Downmix and Convert: of one channel count and format,
// a uniform library's).
Status launch_landing(Landing kind, const std::vector<IngestSpan> &spans) {
  const int channels = spans.front().channels, format = spans.front().format;
  if (kind == Landing::Downmix) {
    std::vector<DownmixSpan> mix;
    for (const IngestSpan &sp : spans) mix.push_back(DownmixSpan{static_cast<const int16_t *>(sp.src[0]), sp.dst, sp.frames});
    return gpu_downmix_device(mix, channels, false);
  }
  if (kind == Landing::Convert) {
    std::vector<ConvertSpan> convert(spans.size());
    for (size_t i = 0; i < spans.size(); i++) {
      std::memcpy(convert[i].src, spans[i].src, sizeof(convert[i].src));
      convert[i].dst = spans[i].dst;
      convert[i].frames = spans[i].frames;
    }
    return gpu_convert_device(convert, channels, format, channels > 2, false);  // 3-8 channels: the down-mix fused in
  }
  return kind == Landing::Rematrix ? gpu_rematrix_device(spans, false) : gpu_ingest_device(spans, false);
}

// set_pcm / set_pcm_device: every window that needs a kernel on its way lands in its place in the resident PCM.  The
// plan is format_plan.h's -- pieces of whole 16-frame groups or of whole output tiles of the window's own rate, batches
// of at most 2 GiB of staging (NEEDLE_HIP_MAX_BATCH_VALUES values, for tests).  Host windows are staged raw, every plane
// 16-byte aligned; device windows are read in place.  Per batch: one upload, one landing launch (a library has one kind
// of landing, format_windows) that writes 11025 Hz windows straight into the resident PCM and the others into staging,
// and one resampler launch per distinct (rate, channels) among those; a window without a landing is resampled out of
// its raw samples, staged or the caller's.  All in library-stream order; the caller synchronises.
Status land_windows(NeedleHipLibrary *lib, const std::vector<FormatWindow> &windows, bool from_host, DeviceBuffer<int16_t> *stage) {
  std::map<int, ResampleTiling> tilings;
  Status s;
  for (const FormatWindow &w : windows)
    if (w.rate != kSampleRate && !tilings.count(w.rate) && !(s = resample_tiling(w.rate, w.out_channels, &tilings[w.rate])).ok()) return s;
  bool count_values = false;
  const uint64_t limit = batch_limit(&count_values);
  FormatPlan plan;
  if (!(s = format_plan_pieces(windows, tilings, from_host, limit, count_values, &plan)).ok()) return s;
  if (plan.capacity && !(s = stage->reserve(plan.capacity)).ok()) return s;
  std::vector<const void *> up_src;
  std::vector<size_t> up_bytes;
  std::vector<uint64_t> up_off;
  std::map<Landing, std::vector<IngestSpan>> land;
  std::map<std::pair<int, int>, std::vector<ResampleSpan>> spans;  // by (rate, channels)
  auto flush = [&]() -> Status {  // the next batch's copies follow these kernels in stream order
    Status fs = up_src.empty() ? Status::Ok() : gpu_upload_raw(up_src, up_bytes, up_off, stage->ptr);
    for (auto &l : land)
      if (fs.ok()) fs = launch_landing(l.first, l.second);
    for (auto &rs : spans)
      if (fs.ok()) fs = gpu_resample_device(nullptr, rs.second, rs.first.second, rs.first.first, lib->d_pcm.ptr, false);
    up_src.clear();
    up_bytes.clear();
    up_off.clear();
    land.clear();
    spans.clear();
    return fs;
  };
  size_t batch = 0;
  for (const FormatPiece &pc : plan.pieces) {
    if (pc.batch != batch) {
      if (!(s = flush()).ok()) return s;
      batch = pc.batch;
    }
    const FormatWindow &w = windows[pc.window];
    const uint64_t n = pc.p1 - pc.p0, W = sample_format_width(w.format);
    const size_t P = sample_format_planes(w.format, w.channels);
    const uint64_t per_frame = P == 1 ? (uint64_t)w.channels : 1;  // samples of one plane per frame
    IngestSpan in{};
    in.frames = n;
    in.channels = w.channels;
    in.format = w.format;
    in.mix = w.mix;
    for (size_t c = 0; c < P; c++) {
      const uint8_t *from = static_cast<const uint8_t *>(w.src[c]) + pc.p0 * per_frame * W;  // the piece in the caller's buffer
      if (from_host) {
        up_src.push_back(from);
        up_bytes.push_back(n * per_frame * W);
        up_off.push_back(pc.raw_off + c * pc.plane_units);
        in.src[c] = stage->ptr + pc.raw_off + c * pc.plane_units;
      } else {
        in.src[c] = from;
      }
    }
    const int16_t *landed = static_cast<const int16_t *>(in.src[0]);  // no landing: the raw s16 itself
    if (w.landing != Landing::None) {
      in.dst = w.rate != kSampleRate ? stage->ptr + pc.mono_off : lib->d_pcm.ptr + w.dst + pc.p0 * (uint64_t)w.out_channels;
      landed = in.dst;
      land[w.landing].push_back(in);
    }
    if (w.rate != kSampleRate) {
      ResampleSpan sp{0, w.frames, w.dst};
      sp.src = landed;
      sp.t0 = pc.t0;
      sp.t1 = pc.t1;
      sp.p0 = pc.p0;
      sp.p1 = pc.p1;
      spans[{w.rate, w.out_channels}].push_back(sp);
    }
  }
  return flush();
}

// needle_hip_library_set_pcm (from_host) and needle_hip_library_set_pcm_device
NeedleError set_pcm_from(NeedleHipLibrary *lib, const int16_t *const *pcm, const size_t *num_values, int channels, bool from_host) {
  if (!lib || !pcm || !num_values) return NeedleError_NullArgument;
  if (!call_channels_ok(lib, channels)) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const void *> planes;
    std::vector<size_t> len;
    std::vector<uint64_t> dst;
    uint64_t total = 0;
    std::vector<size_t> video_of;
    Status s = check_mix_channels(lib, channels);
    if (s.ok()) s = plan_windows(lib, reinterpret_cast<const void *const *>(pcm), num_values, channels, true, &planes, &len, &dst, nullptr, &total, &video_of);
    if (!s.ok()) return report(s);
    if (!(s = lib->d_pcm.reserve(std::max<uint64_t>(total, 1))).ok()) return report(s);
    hipStream_t stream = library_stream();
    DeviceBuffer<int16_t> stage;  // (freed after the drain below)
    const std::vector<FormatWindow> windows = format_windows(lib, channels, planes, len, &dst, video_of);
    // 1-2 channel s16 at 11025 Hz without a mix is resident as it is: nothing to stage, nothing to launch
    const bool as_it_is = !windows.empty() && windows[0].landing == Landing::None && windows[0].rate == kSampleRate;
    if (!as_it_is) {
      s = land_windows(lib, windows, from_host, &stage);
    } else if (from_host) {
      s = gpu_upload_pcm(as_s16(planes), len, dst, lib->d_pcm.ptr);
    } else {
      for (size_t i = 0; i < len.size() && s.ok(); i++)  // the search windows only, device to device, in stream order
        if (hipMemcpyAsync(lib->d_pcm.ptr + dst[i], planes[i], len[i] * sizeof(int16_t), hipMemcpyDeviceToDevice, stream) != hipSuccess)
          s = Status::Make(NeedleError_Unknown, "device-to-device PCM copy failed");
    }
    // also on the error path: copies and kernels already enqueued read the caller's buffers asynchronously
    const bool drained = hipStreamSynchronize(stream) == hipSuccess;
    if (!s.ok()) return report(s);
    if (!drained) return report(Status::Make(NeedleError_Unknown, "PCM transfer failed"));
    lib->have_pcm = true;
    lib->pcm_resident = true;
    return NeedleError_Ok;
  });
}
}  // namespace

extern "C" {

enum NeedleError needle_hip_library_set_pcm(NeedleHipLibrary *lib, const int16_t *const *pcm, const size_t *num_values,
                                            int channels) {
  return set_pcm_from(lib, pcm, num_values, channels, true);
}

enum NeedleError needle_hip_library_set_pcm_device(NeedleHipLibrary *lib, const int16_t *const *d_pcm,
                                                   const size_t *num_values, int channels) {
  return set_pcm_from(lib, d_pcm, num_values, channels, false);
}

enum NeedleError needle_hip_library_stream_pcm(NeedleHipLibrary *lib, const int16_t *const *pcm, const size_t *num_values,
                                               int channels) {
  if (!lib || !pcm || !num_values) return NeedleError_NullArgument;
  if (!call_channels_ok(lib, channels)) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const void *> planes;
    std::vector<size_t> len;
    std::vector<uint64_t> rows;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<size_t> video_of;
    Status s = check_mix_channels(lib, channels);
    if (s.ok()) s = plan_windows(lib, reinterpret_cast<const void *const *>(pcm), num_values, channels, false, &planes, &len, nullptr, &rows, nullptr, &video_of);
    if (!s.ok()) return report(s);
    for (uint64_t &r : rows) r *= lib->stride;  // kept items of a window go straight to its arena row
    const auto t1 = std::chrono::steady_clock::now();
    const std::vector<const int16_t *> src = as_s16(planes);
    s = lib->has_formats ? gpu_fingerprint_formats(format_windows(lib, channels, planes, len, nullptr, video_of), lib->any_mix, lib->step, nullptr, lib->arena, &rows)
        : lib->format != NEEDLE_HIP_SAMPLE_S16 || lib->has_mix
            ? gpu_fingerprint_streamed_device_format(planes, len, channels, lib->format, lib->step, lib->arena, rows, lib->rate,
                                                     lib->has_mix ? &lib->mix : nullptr)
            : gpu_fingerprint_streamed_device(src, len, channels, lib->step, lib->arena, rows, lib->rate);
    if (!s.ok()) return report(s);
    if (getenv("NEEDLE_HIP_TRACE"))
      std::fprintf(stderr, "[needle_hip] stream_pcm: windows planned in %.2f ms, %zu windows streamed in %.2f ms\n",
                   std::chrono::duration<double, std::milli>(t1 - t0).count(), src.size(),
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
    lib->have_pcm = true;
    lib->pcm_resident = false;
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_library_analyze(NeedleHipLibrary *lib, size_t first, size_t count, bool sync) {
  if (!lib) return NeedleError_NullArgument;
  if (!lib->have_pcm || first > lib->n || count > lib->n - first) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    std::vector<StreamSpan> spans;
    const size_t R = lib->regions();
    for (size_t row = first * R; row < (first + count) * R; row++) {
      const Window &w = lib->win[row];
      if (w.pcm_off == ~0ull)
        return report(Status::Make(NeedleError_InvalidArgument, "video " + std::to_string(row / R) + " has no PCM on this rank"));
      spans.push_back(StreamSpan{w.pcm_off, w.values, (uint64_t)row * lib->stride});
    }
    Status s = gpu_fingerprint_device(lib->d_pcm.ptr, spans, lib->channels, lib->step, lib->arena, sync);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_library_hash_arena(NeedleHipLibrary *lib, uint32_t **d_arena, size_t *stride) {
  if (!lib || !d_arena || !stride) return NeedleError_NullArgument;
  if (!lib->have_pcm) return NeedleError_InvalidArgument;
  *d_arena = lib->arena;
  *stride = lib->stride;
  return NeedleError_Ok;
}

size_t needle_hip_library_rows_per_video(const NeedleHipLibrary *lib) { return lib ? lib->regions() : 0; }

enum NeedleError needle_hip_library_use_hash_arena(NeedleHipLibrary *lib, uint32_t *d_arena, size_t rows, size_t stride) {
  if (!lib || !d_arena) return NeedleError_NullArgument;
  if (!lib->have_pcm || rows < lib->rows() || stride < lib->stride) return NeedleError_InvalidArgument;
  if ((uint64_t)rows * stride > UINT32_MAX) return NeedleError_InvalidArgument;
  lib->arena = d_arena;
  lib->arena_rows = rows;
  lib->stride = stride;
  lib->d_arena.release();
  return NeedleError_Ok;
}

size_t needle_hip_library_num_pairs(const NeedleHipLibrary *lib) { return lib ? lib->pairs() : 0; }

enum NeedleError needle_hip_library_search(NeedleHipLibrary *lib, const struct NeedleAudioComparator *comparator,
                                           size_t first_pair, size_t num_pairs, NeedleHipRun *d_runs,
                                           uint32_t capacity, uint32_t *d_count, bool sync) {
  if (!lib || !comparator || !d_runs || !d_count) return NeedleError_NullArgument;
  const size_t np = lib->pairs();
  if (!lib->have_pcm || first_pair > np || num_pairs > np - first_pair) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    const auto t_enter = std::chrono::steady_clock::now();
    const Comparator &cmp = comparator_of(comparator);
    if (cmp.include_endings() && !lib->endings)  // comparator.rs:271-273
      return report(Status::Make(NeedleError_Unknown, "no ending hash data present"));
    const size_t R = lib->regions(), Rc = cmp.include_endings() ? 2 : 1;
    std::vector<NeedleHipSeq> seqs(lib->rows());
    for (size_t row = 0; row < lib->rows(); row++)
      seqs[row] = NeedleHipSeq{(uint32_t)(row * lib->stride), lib->win[row].kept};
    // per-row minimum run length for the duration tests (it depends on the kept length only: the seek offset
    // of an ending window cancels in ts[i] - ts[i-L])
    if (lib->min_len.size() != lib->rows() || lib->min_len_for[0] != cmp.min_opening_duration() ||
        lib->min_len_for[1] != cmp.min_ending_duration()) {
      lib->min_len.assign(lib->rows(), 0);
      for (size_t row = 0; row < lib->rows(); row++) {
        const bool opening = row % R == 0;
        lib->min_len[row] = row >= R && lib->win[row].kept == lib->win[row - R].kept
                                ? lib->min_len[row - R]
                                : cmp.min_run_length_for(lib->timestamps(lib->win[row].kept), opening);
      }
      lib->min_len_for[0] = cmp.min_opening_duration();
      lib->min_len_for[1] = cmp.min_ending_duration();
      lib->problems_for[0] = ~(size_t)0;
    }
    std::vector<NeedleHipProblem> &problems = lib->problems;
    const bool cached = lib->problems_for[0] == first_pair && lib->problems_for[1] == num_pairs && lib->problems_for[2] == Rc;
    if (!cached) {
      lib->problems_for[0] = ~(size_t)0;  // not valid until it is complete
      problems.clear();
      problems.reserve(num_pairs * Rc);
      // (i, j) of the range's first pair, then stepped: i-major over the videos, or -- grouped -- over a group's members
      // (ranks ra < rb of group g) and on to the next group that has a pair
      const GroupTables *gt = lib->groups.get();
      size_t i = 0, j = 0;
      uint32_t g = 0, ra = 0, rb = 1;
      if (num_pairs && !gt) pair_at(lib->n, first_pair, &i, &j);
      if (num_pairs && gt) {
        uint32_t a = 0, b = 0;
        if (!grouped_pair_at(gt->view(), first_pair, &a, &b)) return report(Status::Make(NeedleError_Unknown, "internal error: no such grouped pair"));
        i = a;
        j = b;
        g = gt->group_of[a];
        ra = gt->rank_of[a];
        rb = gt->rank_of[b];
      }
      for (size_t p = first_pair; p < first_pair + num_pairs; p++) {
        for (size_t r = 0; r < Rc; r++) {
          if (r == 1 && (lib->win[i * R + 1].kept == 0 || lib->win[j * R + 1].kept == 0))  // comparator.rs:271-273
            return report(Status::Make(NeedleError_Unknown, "no ending hash data present"));
          const uint32_t a = lib->min_len[i * R + r], b = lib->min_len[j * R + r];
          if (a == 0 || b == 0) continue;
          problems.push_back(NeedleHipProblem{(uint32_t)(i * R + r), (uint32_t)(j * R + r), std::max(a, b),
                                              (uint32_t)(p * Rc + r)});
        }
        if (!gt) {
          if (++j == lib->n) j = ++i + 1;  // next pair in i-major order
          continue;
        }
        if (p + 1 == first_pair + num_pairs) break;
        if (++rb == gt->size[g]) rb = ++ra + 1;
        if (rb >= gt->size[g]) {  // the group's last pair is behind (p + 1 is a pair: there is a next group with one)
          do g++;
          while (gt->size[g] < 2);
          ra = 0;
          rb = 1;
        }
        i = gt->members[gt->first[g] + ra];
        j = gt->members[gt->first[g] + rb];
      }
      lib->problems_for[0] = first_pair;
      lib->problems_for[1] = num_pairs;
      lib->problems_for[2] = Rc;
    }
    // a download that still reads this run buffer (on the download stream) has to finish before it is overwritten
    for (NeedleHipLibrary::Fetch &f : lib->fetch)
      if (f.pending && (f.d_runs == d_runs || f.d_count == d_count) &&
          hipStreamWaitEvent(library_stream(), f.done, 0) != hipSuccess)
        return report(Status::Make(NeedleError_Unknown, "stream wait failed"));
    const auto t_built = std::chrono::steady_clock::now();
    const bool count_is_zero = lib->count_zeroed == d_count;
    lib->count_zeroed = nullptr;
    if (lib->groups && lib->pairs() == 0) {  // a labelling without any pair: nothing is scanned, the count is cleared
      if ((!count_is_zero && hipMemsetAsync(d_count, 0, sizeof(uint32_t), library_stream()) != hipSuccess) ||
          (sync && hipStreamSynchronize(library_stream()) != hipSuccess))
        return report(Status::Make(NeedleError_Unknown, "clearing the run count failed"));
      return NeedleError_Ok;
    }
    Status s = gpu_hamming_runs_device(lib->arena, seqs.data(), seqs.size(), problems.data(), problems.size(),
                                       cmp.hash_match_threshold(), d_runs, capacity, d_count, sync, count_is_zero);
    if (getenv("NEEDLE_HIP_TRACE"))
      std::fprintf(stderr, "[needle_hip] search enqueue: %zu problems built in %.2f ms, launched in %.2f ms\n",
                   problems.size(), std::chrono::duration<double, std::milli>(t_built - t_enter).count(),
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_built).count());
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_library_fetch_runs_begin(NeedleHipLibrary *lib, int slot, const NeedleHipRun *d_runs,
                                                     const uint32_t *d_count, uint32_t max_runs) {
  if (!lib || !d_runs || !d_count) return NeedleError_NullArgument;
  if (slot < 0 || slot > 1 || max_runs == 0) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    NeedleHipLibrary::Fetch &f = lib->fetch[slot];
    if (f.pending) return report(Status::Make(NeedleError_InvalidArgument, "fetch slot still pending"));
    const size_t bytes = 16 + (size_t)max_runs * sizeof(NeedleHipRun);
    if (f.max_runs < max_runs) {
      if (f.host) (void)hipHostFree(f.host);
      f.host = nullptr;
      if (hipHostMalloc(&f.host, bytes, hipHostMallocDefault) != hipSuccess)
        return report(Status::Make(NeedleError_Unknown, "pinned allocation failed"));
      f.max_runs = max_runs;
    }
    if (!f.done && hipEventCreateWithFlags(&f.done, hipEventDisableTiming) != hipSuccess)
      return report(Status::Make(NeedleError_Unknown, "event creation failed"));
    if (!f.ready && hipEventCreateWithFlags(&f.ready, hipEventDisableTiming) != hipSuccess)
      return report(Status::Make(NeedleError_Unknown, "event creation failed"));
    // the copies run on the download stream, behind the search that was just enqueued on the library stream
    hipStream_t stream = library_stream(), down = download_stream();
    if (hipEventRecord(f.ready, stream) != hipSuccess || hipStreamWaitEvent(down, f.ready, 0) != hipSuccess ||
        hipMemcpyAsync(f.host, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, down) != hipSuccess ||
        hipMemcpyAsync(static_cast<char *>(f.host) + 16, d_runs, (size_t)max_runs * sizeof(NeedleHipRun),
                       hipMemcpyDeviceToHost, down) != hipSuccess ||
        hipEventRecord(f.done, down) != hipSuccess)
      return report(Status::Make(NeedleError_Unknown, "asynchronous run download failed"));
    f.d_runs = d_runs;
    f.d_count = d_count;
    f.pending = true;
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_library_fetch_runs_end(NeedleHipLibrary *lib, int slot, const NeedleHipRun **runs,
                                                   uint32_t *num_runs) {
  if (!lib || !runs || !num_runs) return NeedleError_NullArgument;
  if (slot < 0 || slot > 1 || !lib->fetch[slot].pending) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    NeedleHipLibrary::Fetch &f = lib->fetch[slot];
    if (hipEventSynchronize(f.done) != hipSuccess) return report(Status::Make(NeedleError_Unknown, "run download failed"));
    f.pending = false;
    *num_runs = *static_cast<const uint32_t *>(f.host);  // total found; > max_runs means the list was truncated
    *runs = reinterpret_cast<const NeedleHipRun *>(static_cast<const char *>(f.host) + 16);
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_library_finalize(NeedleHipLibrary *lib, const struct NeedleAudioComparator *comparator,
                                             const NeedleHipRun *runs, size_t num_runs,
                                             NeedleHipSearchResult *results) {
  if (!lib || !comparator || (!runs && num_runs) || !results) return NeedleError_NullArgument;
  if (!lib->have_pcm) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    const Comparator &cmp = comparator_of(comparator);
    const std::vector<const FrameHashesData *> fh = lib->shell_pointers();
    std::vector<VideoResult> res;
    const auto t0 = std::chrono::steady_clock::now();
    Status s = cmp.results_from_runs(fh, runs, num_runs, false, false, false, &res, 0, ~(size_t)0, nullptr, lib->groups.get());
    if (getenv("NEEDLE_HIP_TRACE"))
      std::fprintf(stderr, "[needle_hip] epilogue %zu runs: %.1f us\n", num_runs,
                   std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    if (!s.ok()) return report(s);
    for (size_t v = 0; v < lib->n; v++) fill_c_result(res[v], &results[v]);
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_library_frame_hashes(NeedleHipLibrary *lib, size_t index, FrameHashes **output) {
  if (!lib || !output) return NeedleError_NullArgument;
  if (!lib->have_pcm || index >= lib->n) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    const size_t R = lib->regions();
    FrameHashesData fh;
    hipStream_t stream = library_stream();
    for (size_t r = 0; r < R; r++) {
      const Window &w = lib->win[index * R + r];
      std::vector<uint32_t> host(w.kept);
      if (!host.empty() &&
          (hipMemcpyAsync(host.data(), lib->arena + (index * R + r) * lib->stride, host.size() * sizeof(uint32_t),
                          hipMemcpyDeviceToHost, stream) != hipSuccess ||
           hipStreamSynchronize(stream) != hipSuccess))
        return report(Status::Make(NeedleError_Unknown, "hash arena download failed"));
      std::vector<HashTs> ts = lib->window_timestamps(w);
      for (size_t k = 0; k < host.size(); k++) ts[k].hash = host[k];
      (r == 0 ? fh.opening : fh.ending) = std::move(ts);
    }
    fh.hash_duration = lib->hash_duration;
    *output = make_frame_hashes(std::move(fh));
    return NeedleError_Ok;
  });
}

}  // extern "C"

// ---- the whole job, across the communicator ------------------------------------------------------------------------
namespace {

// The rows and columns of the arena that rank `rank`'s flat block meets: f(row, first column, end column), columns
// clipped to the row's kept hashes (the rest of a row is padding).
template <typename F>
void for_rows_of_block(const NeedleHipLibrary *lib, int world, int rank, F &&f) {
  const size_t B = lib->flat_block(world), begin = (size_t)rank * B, end = begin + B;
  if (!lib->stride) return;
  for (size_t row = begin / lib->stride; row < lib->rows() && row * lib->stride < end; row++) {
    const size_t r0 = row * lib->stride;
    const size_t c0 = begin > r0 ? begin - r0 : 0, c1 = std::min<size_t>(std::min(end - r0, lib->stride), lib->win[row].kept);
    if (c0 < c1) f(row, c0, c1);
  }
}

// The streams this rank's share of the fingerprinting is made of: whole windows without a communicator, otherwise per row
// of its block the sub-window of PCM the block's columns depend on, hashes straight to their places.
Status block_spans(const NeedleHipLibrary *lib, int world, int rank, std::vector<StreamSpan> *spans) {
  if (world <= 1) {
    for (size_t row = 0; row < lib->rows(); row++) {
      const Window &w = lib->win[row];
      if (w.pcm_off == ~0ull)
        return Status::Make(NeedleError_InvalidArgument, "video " + std::to_string(row / lib->regions()) + " has no PCM on this rank");
      spans->push_back(StreamSpan{w.pcm_off, w.values, (uint64_t)row * lib->stride});
    }
    return Status::Ok();
  }
  Status bad;
  for_rows_of_block(lib, world, rank, [&](size_t row, size_t c0, size_t c1) {
    const Window &w = lib->win[row];
    if (w.pcm_off == ~0ull) {
      bad = Status::Make(NeedleError_InvalidArgument, "video " + std::to_string(row / lib->regions()) +
                                                          " has no PCM on this rank (needle_hip_library_rank_videos names the videos a rank needs)");
      return;
    }
    // hashes c0 .. c1-1 = raw items c0 step .. (c1 - 1) step = frames c0 step .. (c1 - 1) step + 19
    const uint64_t x0 = (uint64_t)c0 * lib->step, frames = (uint64_t)(c1 - 1 - c0) * lib->step + 20;
    const uint64_t samples = (frames - 1) * (uint64_t)kHop + (uint64_t)kFrameSize;
    spans->push_back(StreamSpan{w.pcm_off + x0 * (uint64_t)kHop * (uint64_t)lib->channels, samples * (uint64_t)lib->channels,
                                (uint64_t)row * lib->stride + c0});
  });
  return bad;
}

// Fingerprints this rank's block.
NeedleError analyze_flat_block(NeedleHipLibrary *lib, int world, int rank, int slot, uint32_t *zero_word) {
  std::vector<StreamSpan> spans;
  bool zeroed = false;
  lib->count_zeroed = nullptr;
  Status s = block_spans(lib, world, rank, &spans);
  if (!s.ok()) return report(s);
  if (spans.empty()) return NeedleError_Ok;
  // `slot`: the job slot is the pipeline depth -- job k + 1's STFT may overlap the tail of job k (common.h)
  s = gpu_fingerprint_device(lib->d_pcm.ptr, spans, lib->channels, lib->step, lib->arena, false, nullptr, nullptr, 0, slot,
                             zero_word, &zeroed);
  if (s.ok() && zeroed) lib->count_zeroed = zero_word;
  return s.ok() ? NeedleError_Ok : report(s);
}

// ---- A library job: stages that execute a plan.  What the ranks send each other is decided in job_plan.h (plan_job, judge);
// nothing below decides a size, an offset or a form.

// Every environment hook of the job path.  Read again at every job_begin, every repeat and every job_end: the tests change
// them between the jobs of one process.
JobHook hook(const char *name) {
  const char *e = getenv(name);
  return JobHook{e != nullptr, e ? atoi(e) : 0};
}
JobSwitches job_switches() {
  JobSwitches sw;
  sw.device_epilogue = hook("NEEDLE_HIP_DEVICE_EPILOGUE");
  sw.shard_epilogue = hook("NEEDLE_HIP_SHARD_EPILOGUE");
  sw.shard_epilogue_pairs = hook("NEEDLE_HIP_SHARD_EPILOGUE_PAIRS");
  sw.directed_runs = hook("NEEDLE_HIP_DIRECTED_RUNS");
  sw.head_runs = hook("NEEDLE_HIP_HEAD_RUNS");
  sw.slab_runs = hook("NEEDLE_HIP_SLAB_RUNS");
  sw.test_directed_cap = hook("NEEDLE_HIP_TEST_DIRECTED_CAP");
  sw.test_epilogue_fail_rank = hook("NEEDLE_HIP_TEST_EPILOGUE_FAIL_RANK");
  return sw;
}

using Job = NeedleHipLibrary::Job;
uint32_t *slab_count_word(uint8_t *slab) { return reinterpret_cast<uint32_t *>(slab); }
NeedleHipRun *slab_runs_of(uint8_t *slab) { return reinterpret_cast<NeedleHipRun *>(slab + kSlabHeader); }
const NeedleHipRun *slab_runs_of(const void *slab) {
  return reinterpret_cast<const NeedleHipRun *>(static_cast<const uint8_t *>(slab) + kSlabHeader);
}

// Events and buffers for a plan: this rank's slab, the heads of all ranks on the device and pinned.  Grow only.
Status job_buffers(Job::Buffers &b, const JobPlan &p) {
  if (!b.searched) NEEDLE_HIP_TRY(hipEventCreateWithFlags(&b.searched, hipEventDisableTiming));
  if (!b.done) NEEDLE_HIP_TRY(hipEventCreateWithFlags(&b.done, hipEventDisableTiming));
  Status s;
  if (b.slab_runs != p.slab_runs || b.world != p.shape.world) {
    b.slab_runs = p.slab_runs;
    b.world = p.shape.world;
    b.d_slabs.release();
    if (!(s = b.d_slabs.reserve(slab_bytes(p.slab_runs))).ok()) return s;
  }
  if (p.shape.world > 1 && !(s = b.d_heads.reserve(p.pinned_bytes)).ok()) return s;
  if (p.pinned_bytes > b.host.bytes) s = b.host.reserve(p.pinned_bytes + p.pinned_bytes / 4);
  return s;
}

// Stage 1: the plan of this attempt, from what the last finished job -- or this job's last attempt -- left, and buffers for it.
// On a repeat the WHOLE plan is made again, so the form can change between a job's first attempt and its repeat.
NeedleError job_plan_stage(NeedleHipLibrary *lib, const NeedleAudioComparator *comparator, Job &j, uint32_t keep_head = 0) {
  JobShape shape;
  shape.n = lib->n;
  shape.arena_regions = lib->regions();
  shape.comparator_regions = comparator_of(comparator).include_endings() ? 2 : 1;
  shape.world = comm_world();
  shape.rank = comm_rank();
  if (lib->groups) shape.pairs = lib->groups->pairs();
  j.planned.plan = plan_job(shape, job_switches(), lib->history, keep_head);
  const JobPlan &p = j.planned.plan;
  lib->history.slab_runs = p.slab_runs;  // (a first slab sticks)
  if (p.directed.cap_consumed) lib->history.dir_cap_forced = true;
  Status s = job_buffers(j.buf, p);
  return s.ok() ? NeedleError_Ok : report(s);
}

// Stage 2: the scan of this rank's pair range into its slab; the download stream waits for it.
NeedleError job_scan(NeedleHipLibrary *lib, const NeedleAudioComparator *comparator, Job &j) {
  const JobPlan &p = j.planned.plan;
  uint8_t *mine = j.buf.d_slabs.ptr;
  NeedleError e = needle_hip_library_search(lib, comparator, p.pair_first, p.pair_count, slab_runs_of(mine), p.slab_runs,
                                            slab_count_word(mine), false);
  if (e != NeedleError_Ok) return e;
  // the form of THIS job's scan, taken as it is enqueued: by job_end the process's last launch may be another job's,
  // with another comparator (threshold) and so another form
  int32_t form = 0;
  uint64_t products = 0;
  gpu_scan_last_launch(&form, &products);
  j.planned.scan_form = (uint32_t)form;
  if (hipEventRecord(j.buf.searched, library_stream()) != hipSuccess || hipStreamWaitEvent(download_stream(), j.buf.searched, 0) != hipSuccess)
    return report(Status::Make(NeedleError_Unknown, "stream ordering failed"));
  return NeedleError_Ok;
}

// Stage 3a, directed exchange: this rank's runs sorted into one block per destination, and the count matrix -- this rank's
// row [runs in its slab, runs directed to rank 0, 1, ...] gathered from every rank and downloaded.  A job without block
// sizes (plan.directed.sized) does this much: it counts, and travels as heads.
Status job_count_directed(NeedleHipLibrary *lib, Job &j) {
  const JobPlan &p = j.planned.plan;
  const DirectedPlan &d = p.directed;
  const int world = p.shape.world;
  const size_t W = (size_t)world, cw = count_words(world);
  hipStream_t down = download_stream();
  uint8_t *mine = j.buf.d_slabs.ptr;
  if (d.refused) return Status::Make(NeedleError_InvalidArgument, "directed run exchange: blocks beyond 4 GiB");
  DirectPlan blocks;
  std::memset(&blocks, 0, sizeof(blocks));
  for (size_t q = 0; q < W; q++) {
    blocks.offset[q] = (uint32_t)d.send_off[q];
    blocks.capacity[q] = d.send_capacity[q];
  }
  Status s = j.buf.d_dir_send.reserve(d.send_total);
  if (s.ok()) s = j.buf.d_dir_counts.reserve(cw * W);
  if (s.ok()) s = j.buf.host_counts.reserve(count_matrix_bytes(world));
  if (s.ok() && lib->groups) s = ensure_device_groups(lib);
  if (s.ok())
    s = gpu_direct_runs(slab_count_word(mine), slab_runs_of(mine), p.slab_runs, (uint32_t)p.shape.n, (uint32_t)p.shape.comparator_regions,
                        (uint32_t)shard_block(p.shape.n, world), world, j.buf.d_dir_send.ptr, blocks, down,
                        lib->groups ? &lib->d_groups.view : nullptr);
  if (!s.ok()) return s;
  uint32_t *row = j.buf.d_dir_counts.ptr + (size_t)p.shape.rank * cw;
  bool ok = hipMemsetAsync(row, 0, cw * sizeof(uint32_t), down) == hipSuccess &&
            hipMemcpyAsync(row, mine, sizeof(uint32_t), hipMemcpyDeviceToDevice, down) == hipSuccess;
  for (size_t q = 0; q < W && ok; q++)
    ok = hipMemcpyAsync(row + 1 + q, j.buf.d_dir_send.ptr + d.send_off[q], sizeof(uint32_t), hipMemcpyDeviceToDevice, down) == hipSuccess;
  if (!ok) return Status::Make(NeedleError_Unknown, "directed run exchange: count row failed");
  if (!(s = comm_all_gather(kSide, row, j.buf.d_dir_counts.ptr, cw * sizeof(uint32_t), down)).ok()) return s;
  if (hipMemcpyAsync(j.buf.host_counts.ptr, j.buf.d_dir_counts.ptr, count_matrix_bytes(world), hipMemcpyDeviceToHost, down) != hipSuccess)
    return Status::Make(NeedleError_Unknown, "directed run exchange: count download failed");
  j.planned.counted = true;
  j.found.comm_bytes[1] += count_matrix_bytes(world);
  return Status::Ok();
}

// Stage 3b: the all-to-all of the blocks.  A librccl without point-to-point transfers says "unsupported" before any transfer,
// on every rank (every rank loads the same library): from here on this library's jobs travel as heads, this one included.
Status job_exchange_directed(NeedleHipLibrary *lib, Job &j) {
  JobPlan &p = j.planned.plan;
  const DirectedPlan &d = p.directed;
  Status s = j.buf.d_dir_recv.reserve(d.recv_total);
  if (!s.ok()) return s;
  s = comm_all_to_all_v(kSide, j.buf.d_dir_send.ptr, d.send_off.data(), d.send_bytes.data(), j.buf.d_dir_recv.ptr, d.recv_off.data(),
                        d.recv_bytes.data(), d.max_block_bytes, download_stream());
  if (s.ok()) {
    j.planned.directed = true;
    j.found.comm_bytes[1] += d.recv_total;
  } else if (s.message.find("unsupported") != std::string::npos) {
    lib->history.dir_unsupported = true;
    p.segments = segment_layout(p, false);
    (void)hipGetLastError();
    return Status::Ok();
  }
  return s;
}

// Stage 4, a job that does not travel directed: what travels is the HEAD of every rank's slab -- its count and as many runs as
// the last job needed plus a margin -- not the slab's capacity: at BASELINE.json configs[4] on 8 GPUs a slab is 24 MB per
// rank and the runs found 13 MB.  The heads land side by side in d_heads and come down in ONE copy; a rank whose count
// exceeds the head is job_end's case (every rank sees every count).  One rank: the head is copied straight out of the slab.
Status job_gather_heads(Job &j) {
  const JobPlan &p = j.planned.plan;
  const uint8_t *src = j.buf.d_slabs.ptr;
  if (p.shape.world > 1) {
    Status s = comm_all_gather(kSide, j.buf.d_slabs.ptr, j.buf.d_heads.ptr, p.head_bytes(), download_stream());
    if (!s.ok()) return s;
    src = j.buf.d_heads.ptr;
    j.found.comm_bytes[1] += p.head_bytes() * (uint64_t)p.shape.world;
  }
  if (hipMemcpyAsync(j.buf.host.ptr, src, p.head_bytes() * (size_t)p.shape.world, hipMemcpyDeviceToHost, download_stream()) != hipSuccess)
    return Status::Make(NeedleError_Unknown, "asynchronous run download failed");
  return Status::Ok();
}

// Stage 5: the device epilogue behind the exchange, its segments as the plan lays them out.  A rank on which it fails
// (workspaces that do not fit, more than 64 ranks) computes the same results on the host from the downloaded run list, for
// the same block of videos: plan.sharded stands (shape_fixed) -- a rank that fell back alone must still meet the others in
// the collective they enter, or not enter one they skip.
Status job_device_epilogue(NeedleHipLibrary *lib, const Comparator &cmp, Job &j) {
  const JobPlan &p = j.planned.plan;
  const int world = p.shape.world;
  Status s = j.buf.host_results.reserve((lib->n + 1) * sizeof(NeedleHipSearchResult));
  if (!s.ok()) return s;
  lib->ensure_row_tables();
  EpilogueJob ej;
  ej.slot = (int)(&j - lib->job);
  ej.n = (uint32_t)lib->n;
  ej.regions = (uint32_t)p.shape.comparator_regions;
  ej.rows_per_video = (uint32_t)lib->regions();
  ej.v0 = (uint32_t)p.video_first;
  ej.v1 = (uint32_t)(p.video_first + p.video_count);
  ej.threshold = cmp.hash_match_threshold();
  ej.include_endings = cmp.include_endings();
  ej.min_opening_duration = cmp.min_opening_duration();
  ej.min_ending_duration = cmp.min_ending_duration();
  ej.time_padding = cmp.time_padding();
  ej.hash_duration = lib->hash_duration;
  ej.num_segments = world;
  const SegmentLayout &seg = p.segments;
  for (int r = 0; r < world && r < 64; r++) {  // (EpilogueJob has 64 segments; a larger world is refused below)
    const uint8_t *slab = seg.kind == SegmentKind::Blocks  ? j.buf.d_dir_recv.ptr + p.directed.recv_off[(size_t)r]
                          : seg.kind == SegmentKind::Heads ? j.buf.d_heads.ptr + (size_t)r * p.head_bytes()
                                                           : j.buf.d_slabs.ptr;
    ej.segment_count[r] = reinterpret_cast<const uint32_t *>(slab);
    ej.segment_runs[r] = slab_runs_of(slab);
    if (seg.kind == SegmentKind::Blocks) ej.segment_capacities[r] = seg.capacities[(size_t)r];
  }
  ej.segment_capacity = seg.capacity;
  ej.max_runs = seg.max_runs;
  ej.row_len = &lib->row_len;
  ej.row_ts = &lib->row_ts;
  ej.row_seek = &lib->row_seek;
  ej.ts = &lib->ts_tables;
  if (lib->groups) {  // the grouped form, for this rank's block of videos (all of them unless sharded)
    ej.groups = lib->groups.get();
    ej.hash_durations = &lib->hash_durations;
    ej.block_wanted = true;
  }
  NeedleHipSearchResult *hr = static_cast<NeedleHipSearchResult *>(j.buf.host_results.ptr);
  s = world <= 64 ? gpu_epilogue_enqueue(ej, download_stream(), hr, reinterpret_cast<uint32_t *>(hr + lib->n))
                  : Status::Make(NeedleError_InvalidArgument, "device epilogue: more than 64 ranks");
  if (p.inject_epilogue_failure) s = Status::Make(NeedleError_Unknown, "device epilogue: failure injected by the test");
  if (!s.ok()) {
    j.planned.device_epilogue = false;
    (void)hipGetLastError();
  }
  return Status::Ok();
}

// Stages 2 to 5 of the planned job: scan, exchange of the runs, download of the counts, epilogue -- all asynchronous.
NeedleError job_enqueue(NeedleHipLibrary *lib, const NeedleAudioComparator *comparator, Job &j) {
  const JobPlan &p = j.planned.plan;
  NeedleError e = job_scan(lib, comparator, j);
  if (e != NeedleError_Ok) return e;
  j.planned.device_epilogue = p.device_epilogue;
  j.planned.counted = j.planned.directed = false;
  j.found.fetched_valid = false;
  Status s;
  if (p.directed.wanted) s = job_count_directed(lib, j);
  if (s.ok() && p.directed.wanted && p.directed.sized) s = job_exchange_directed(lib, j);
  if (s.ok() && !j.planned.directed) s = job_gather_heads(j);
  if (s.ok() && p.device_epilogue) s = job_device_epilogue(lib, comparator_of(comparator), j);
  if (s.ok() && hipEventRecord(j.buf.done, download_stream()) != hipSuccess) s = Status::Make(NeedleError_Unknown, "asynchronous run download failed");
  return s.ok() ? NeedleError_Ok : report(s);
}

// Owner-directed job: the runs this rank received (its own videos' pairs), downloaded once, on demand.
Status fetch_directed(Job &j) {
  if (j.found.fetched_valid) return Status::Ok();
  const JobPlan &p = j.planned.plan;
  const size_t W = (size_t)p.shape.world, rank = (size_t)p.shape.rank;
  const uint32_t *m = static_cast<const uint32_t *>(j.buf.host_counts.ptr);
  auto have = [&](size_t r) { return std::min(directed_count(m, p.shape.world, r, rank), p.directed.cap[r * W + rank]); };
  size_t total = 0, at = 0;
  for (size_t r = 0; r < W; r++) total += have(r);
  j.found.fetched.resize(total);
  for (size_t r = 0; r < W; r++) {
    if (have(r))
      NEEDLE_HIP_TRY(hipMemcpyAsync(j.found.fetched.data() + at, slab_runs_of(j.buf.d_dir_recv.ptr + p.directed.recv_off[r]),
                                    (size_t)have(r) * sizeof(NeedleHipRun), hipMemcpyDeviceToHost, download_stream()));
    at += have(r);
  }
  NEEDLE_HIP_TRY(hipStreamSynchronize(download_stream()));
  j.found.fetched_valid = true;
  return Status::Ok();
}

// job_end, first part: wait for the counts, judge them (job_plan.h), and while something overflowed repeat the job under a new
// plan -- every rank sees the same counts, so every rank repeats or none does.  The scan is deterministic and the arena
// still holds the hashes, whether or not the next job's analyze has run in between (same PCM, same rows).
NeedleError job_settle(NeedleHipLibrary *lib, const NeedleAudioComparator *comparator, Job &j, std::vector<uint32_t> *counts) {
  for (;;) {
    if (hipEventSynchronize(j.buf.done) != hipSuccess) return report(Status::Make(NeedleError_Unknown, "run download failed"));
    const JobPlan &p = j.planned.plan;
    const int world = p.shape.world;
    JobCounts c;
    if (j.planned.counted) c = counts_from_matrix(static_cast<const uint32_t *>(j.buf.host_counts.ptr), world, j.planned.directed);
    if (!j.planned.directed) {  // the heads came down: word 0 of each
      c.slab.resize((size_t)world);
      for (size_t r = 0; r < (size_t)world; r++)
        c.slab[r] = *reinterpret_cast<const uint32_t *>(static_cast<const char *>(j.buf.host.ptr) + r * p.head_bytes());
    }
    JobVerdict v = judge(p, c, lib->history);
    lib->history = std::move(v.history);
    switch (v.next) {
      case JobNext::Done:
        *counts = std::move(c.slab);
        return NeedleError_Ok;
      case JobNext::GrowHead:    // some rank's list is longer than the head that was gathered: head_runs follows last_max_count
      case JobNext::GrowBlocks:  // a block overflowed: the sizes follow the matrix just taken.  (The slab is intact; the scan is repeated all
                                 // the same.  The head alone stays as it was: v.keep_head.)
      case JobNext::GrowSlab:    // some rank found more runs than a slab holds: history.slab_runs grew
        break;
    }
    NeedleError e = job_plan_stage(lib, comparator, j, v.keep_head);
    if (e == NeedleError_Ok) e = job_enqueue(lib, comparator, j);
    if (e != NeedleError_Ok) return e;
    j.found.comm_bytes[3]++;
  }
}

// The run list of all ranks: heads from the pinned buffer, tails (rare: one rank, the first job of a library) straight out of
// its own slab.  A directed job's runs stayed on the devices: each rank holds its own videos' (fetch_directed, on demand),
// and needle_hip_library_job_runs returns that share although job_end's count is the global total.
Status job_collect_runs(Job &j, const std::vector<uint32_t> &counts, const NeedleHipRun **run_list, size_t *total) {
  const JobPlan &p = j.planned.plan;
  const int world = p.shape.world;
  const char *host = static_cast<const char *>(j.buf.host.ptr);
  *total = 0;
  for (int r = 0; r < world; r++) *total += counts[r];
  *run_list = nullptr;
  j.found.merged.clear();
  if (j.planned.directed) return Status::Ok();
  if (world == 1 && counts[0] <= p.head_runs) {  // one rank, everything in the pinned head: no copy of ~100 MB at library scale
    *run_list = slab_runs_of(host);
    return Status::Ok();
  }
  j.found.merged.resize(*total);
  size_t at = 0;
  bool tails = false;
  for (int r = 0; r < world; r++) {
    const uint32_t head = std::min(counts[r], p.head_runs);
    std::memcpy(j.found.merged.data() + at, slab_runs_of(host + (size_t)r * p.head_bytes()), (size_t)head * sizeof(NeedleHipRun));
    if (counts[r] > head) {
      tails = true;
      if (hipMemcpyAsync(j.found.merged.data() + at + head, slab_runs_of(j.buf.d_slabs.ptr + (size_t)r * slab_bytes(p.slab_runs)) + head,
                         (size_t)(counts[r] - head) * sizeof(NeedleHipRun), hipMemcpyDeviceToHost, download_stream()) != hipSuccess)
        return Status::Make(NeedleError_Unknown, "run download failed");
    }
    at += counts[r];
  }
  if (tails && hipStreamSynchronize(download_stream()) != hipSuccess) return Status::Make(NeedleError_Unknown, "run download failed");
  *run_list = j.found.merged.data();
  return Status::Ok();
}

// The order-sensitive per-video epilogue (comparator.rs:583-626) for videos [v0, v0 + vcount): what the device computed
// behind the gather (*device_results), else the host form from the run list -- of a directed job, from the runs this rank
// received.  *epilogue is the epilogue's own outcome: sharded, it travels with the results.  What is returned is a failure
// to fetch the received runs, which ends job_end at once (before the gather of result blocks, as it always did).
Status job_results(NeedleHipLibrary *lib, const Comparator &cmp, Job &j, const NeedleHipRun *run_list, size_t total, size_t v0, size_t vcount,
                   const NeedleHipSearchResult **device_results, std::vector<VideoResult> *res, Status *epilogue) {
  *epilogue = Status::Ok();
  *device_results = nullptr;
  if (j.planned.device_epilogue) {  // (j.buf.done covers its copies)
    *device_results = static_cast<const NeedleHipSearchResult *>(j.buf.host_results.ptr);
    const uint32_t fail = *reinterpret_cast<const uint32_t *>(*device_results + lib->n);
    if (fail & kEpilogueBucketTooLarge) {
      *device_results = nullptr;  // a pair with more runs than one lane should order: the host form below, same block of videos
      note_epilogue_host_fallback("library job", total, vcount);
    } else if (fail != 0) {
      *epilogue = Status::Make(NeedleError_Unknown, "overflow when subtracting durations (time_padding / hash_duration exceed the match end)");
    }
  }
  if (*device_results) return Status::Ok();
  const std::vector<const FrameHashesData *> fh = lib->shell_pointers();
  if (j.planned.directed) {  // this rank's videos' runs are what it received: down they come, once
    Status f = fetch_directed(j);
    if (!f.ok()) return f;
    run_list = j.found.fetched.data();
    total = j.found.fetched.size();
  }
  *epilogue = cmp.results_from_runs(fh, run_list, total, false, false, false, res, v0, v0 + vcount, nullptr, lib->groups.get());
  return Status::Ok();
}

// Sharded epilogue: every rank's block of results, gathered.  An error on one rank must not leave the others waiting in
// the collective: it travels with the results.
Status job_gather_results(NeedleHipLibrary *lib, Job &j, const Status &mine_status, const NeedleHipSearchResult *device_results,
                          const std::vector<VideoResult> &res, NeedleHipSearchResult *results) {
  const JobPlan &p = j.planned.plan;
  const int world = p.shape.world;
  size_t v0 = 0, vcount = 0;
  shard_range(lib->n, world, p.shape.rank, &v0, &vcount);
  struct Block {
    uint64_t failed;
  };
  const size_t block_bytes = sizeof(Block) + shard_block(lib->n, world) * sizeof(NeedleHipSearchResult);
  std::vector<uint8_t> mine(block_bytes, 0), all(block_bytes * (size_t)world, 0);
  reinterpret_cast<Block *>(mine.data())->failed = mine_status.ok() ? 0 : 1;
  if (mine_status.ok() && device_results)
    std::memcpy(mine.data() + sizeof(Block), device_results + v0, vcount * sizeof(NeedleHipSearchResult));
  else if (mine_status.ok())
    for (size_t k = 0; k < vcount; k++) fill_c_result(res[v0 + k], reinterpret_cast<NeedleHipSearchResult *>(mine.data() + sizeof(Block)) + k);
  Status g = comm_all_gather_host(mine.data(), all.data(), block_bytes);
  j.found.comm_bytes[2] += block_bytes * (uint64_t)world;
  if (!mine_status.ok()) return mine_status;
  if (!g.ok()) return g;
  for (int r = 0; r < world; r++) {
    const uint8_t *blk = all.data() + (size_t)r * block_bytes;
    if (reinterpret_cast<const Block *>(blk)->failed) return Status::Make(NeedleError_Unknown, "the epilogue failed on rank " + std::to_string(r));
    size_t f = 0, c = 0;
    shard_range(lib->n, world, r, &f, &c);
    std::memcpy(results + f, blk + sizeof(Block), c * sizeof(NeedleHipSearchResult));
  }
  return Status::Ok();
}

template <typename F>
NeedleError guarded_status(F &&f) {
  return guarded([&]() -> NeedleError {
    Status s = f();
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

}  // namespace

extern "C" {

int needle_hip_comm_rank(void) { return comm_rank(); }
int needle_hip_comm_world_size(void) { return comm_world(); }
const char *needle_hip_comm_backend(void) { return comm_backend(); }

enum NeedleError needle_hip_comm_create_id(uint8_t id[NEEDLE_HIP_COMM_ID_BYTES]) {
  if (!id) return NeedleError_NullArgument;
  return guarded_status([&] { return comm_create_id(id); });
}

enum NeedleError needle_hip_comm_init(const uint8_t id[NEEDLE_HIP_COMM_ID_BYTES], int rank, int world_size) {
  if (!id) return NeedleError_NullArgument;
  return guarded_status([&] { return comm_init(id, rank, world_size); });
}

void needle_hip_comm_finalize(void) { comm_finalize(); }

enum NeedleError needle_hip_comm_barrier(void) {
  return guarded_status([&] { return comm_barrier(); });
}

enum NeedleError needle_hip_comm_all_gather_host(const void *send, void *recv, size_t bytes_per_rank) {
  if ((!send || !recv) && bytes_per_rank) return NeedleError_NullArgument;
  return guarded_status([&] { return comm_all_gather_host(send, recv, bytes_per_rank); });
}

void needle_hip_comm_shard(size_t units, int world_size, int rank, size_t *first, size_t *count) {
  size_t f = 0, c = 0;
  if (world_size >= 1 && rank >= 0 && rank < world_size) shard_range(units, world_size, rank, &f, &c);
  if (first) *first = f;
  if (count) *count = c;
}

enum NeedleError needle_hip_library_rank_videos(const NeedleHipLibrary *lib, const size_t *num_values, int channels, int world_size,
                                                int rank, size_t *first_video, size_t *video_count) {
  if (!lib || !num_values || !first_video || !video_count) return NeedleError_NullArgument;
  if (!call_channels_ok(lib, channels) || world_size < 1 || rank < 0 || rank >= world_size) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    // the geometry plan_windows will arrive at for these lengths, without touching the library
    NeedleHipLibrary plan;
    plan.n = lib->n;
    plan.endings = lib->endings;
    plan.step = lib->step;
    const size_t R = plan.regions();
    plan.win.assign(plan.rows(), Window{});
    uint32_t max_kept = 0;
    const VideoLayouts video(lib, channels);
    for (size_t v = 0; v < plan.n; v++) {
      size_t open_samples = 0, end_first = 0;
      ns_t seek = 0;
      const VideoLayout l = video(v);
      const size_t samples = num_values[v] / (size_t)l.channels;
      Status s = Analyzer::windows(samples, l.rate, lib->opening_pct, lib->ending_pct, &open_samples, &end_first, &seek);
      if (!s.ok()) return report(s);
      for (size_t r = 0; r < R; r++) {
        plan.win[v * R + r].kept = (uint32_t)num_kept(resident_samples(r == 0 ? open_samples : samples - end_first, l.rate), lib->step);
        max_kept = std::max(max_kept, plan.win[v * R + r].kept);
      }
    }
    size_t tiles_per_row = std::max<size_t>(1, ((size_t)max_kept + 63) / 64);
    while (world_size > 1 && (plan.rows() * tiles_per_row) % (size_t)world_size) tiles_per_row++;
    plan.stride = 64 * tiles_per_row;
    size_t lo = plan.n, hi = 0;
    if (world_size == 1) {
      lo = 0;
      hi = plan.n;
    } else {
      for_rows_of_block(&plan, world_size, rank, [&](size_t row, size_t, size_t) {
        lo = std::min(lo, row / R);
        hi = std::max(hi, row / R + 1);
      });
    }
    *first_video = lo < hi ? lo : 0;
    *video_count = lo < hi ? hi - lo : 0;
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_library_job_begin(NeedleHipLibrary *lib, const struct NeedleAudioComparator *comparator, int slot) {
  if (!lib || !comparator) return NeedleError_NullArgument;
  if (slot < 0 || slot > 1 || !lib->have_pcm) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    Job &j = lib->job[slot];
    if (j.pending) return report(Status::Make(NeedleError_InvalidArgument, "job slot still pending"));
    const int world = comm_world(), rank = comm_rank();
    j.found.last_runs = nullptr;
    j.found.last_total = 0;
    std::fill(j.found.comm_bytes, j.found.comm_bytes + 4, 0);
    if (!lib->flat_shardable(world))
      return report(Status::Make(NeedleError_InvalidArgument,
                                 "the hash arena does not divide into this communicator's blocks: call needle_hip_library_set_pcm "
                                 "after needle_hip_comm_init (or adopt an arena of rows x stride with rows * stride / 64 a multiple of the world size)"));
    // (the plan and the run slabs first: the analyze step's last kernel clears this job's run counter)
    NeedleError e = job_plan_stage(lib, comparator, j);
    if (e != NeedleError_Ok) return e;
    // 1. fingerprint this rank's block of HASHES (NeedleHipLibrary::flat_block) into the arena (analyzer.rs:437-445
    // across GPUs).  (After needle_hip_library_stream_pcm the rows are already there: the PCM was fingerprinted as it
    // was uploaded.)
    lib->count_zeroed = nullptr;
    e = lib->pcm_resident ? analyze_flat_block(lib, world, rank, slot, slab_count_word(j.buf.d_slabs.ptr)) : NeedleError_Ok;
    if (e != NeedleError_Ok) return e;
    // 2. every rank gets every hash: one in-place all-gather of the equal blocks, in stream order
    if (comm_get()) {
      const size_t block_bytes = lib->flat_block(world) * sizeof(uint32_t);
      Status s = comm_all_gather(kData, reinterpret_cast<const uint8_t *>(lib->arena) + (size_t)rank * block_bytes, lib->arena,
                                 block_bytes, library_stream());
      if (!s.ok()) return report(s);
      j.found.comm_bytes[0] += block_bytes * (uint64_t)world;
    }
    // 3. + 4. scan this rank's pair range (comparator.rs:549-564 across GPUs), exchange the run lists, enqueue the epilogue
    if ((e = job_enqueue(lib, comparator, j)) != NeedleError_Ok) return e;
    j.pending = true;
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_library_job_end(NeedleHipLibrary *lib, const struct NeedleAudioComparator *comparator, int slot,
                                            NeedleHipSearchResult *results, size_t *num_runs) {
  if (!lib || !comparator || !results) return NeedleError_NullArgument;
  if (slot < 0 || slot > 1 || !lib->job[slot].pending) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    Job &j = lib->job[slot];
    std::vector<uint32_t> counts;
    NeedleError e = job_settle(lib, comparator, j, &counts);
    if (e != NeedleError_Ok) return e;
    j.pending = false;
    const JobPlan &p = j.planned.plan;
    const NeedleHipRun *run_list = nullptr;
    size_t total = 0;
    Status s = job_collect_runs(j, counts, &run_list, &total);
    if (!s.ok()) return report(s);
    if (num_runs) *num_runs = total;
    j.found.last_runs = run_list;
    j.found.last_total = total;
    // 5. the per-video epilogue: every rank for all videos while that is cheaper than another collective, otherwise each
    // rank for its own block of videos + one all-gather of results
    const bool sharded = sharded_at_end(p, hook("NEEDLE_HIP_SHARD_EPILOGUE"), total);
    size_t v0 = 0, vcount = lib->n;
    if (sharded) shard_range(lib->n, p.shape.world, p.shape.rank, &v0, &vcount);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<VideoResult> res;
    const NeedleHipSearchResult *device_results = nullptr;
    Status fetched = job_results(lib, comparator_of(comparator), j, run_list, total, v0, vcount, &device_results, &res, &s);
    j.found.ran_device_epilogue = device_results != nullptr;
    j.found.ran_sharded = sharded;
    if (!fetched.ok()) return report(fetched);
    if (getenv("NEEDLE_HIP_TRACE"))
      std::fprintf(stderr, "[needle_hip] rank %d epilogue %zu runs, videos [%zu, %zu): %.1f us\n", p.shape.rank, total, v0, v0 + vcount,
                   std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    if (sharded) s = job_gather_results(lib, j, s, device_results, res, results);
    if (!s.ok()) return report(s);
    if (!sharded && device_results) std::memcpy(results, device_results, lib->n * sizeof(NeedleHipSearchResult));
    if (!sharded && !device_results)
      for (size_t v = 0; v < lib->n; v++) fill_c_result(res[v], &results[v]);
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_library_job_runs(const NeedleHipLibrary *lib, int slot, const NeedleHipRun **runs, size_t *num_runs) {
  if (!lib || !runs || !num_runs) return NeedleError_NullArgument;
  if (slot < 0 || slot > 1 || lib->job[slot].pending) return NeedleError_InvalidArgument;
  if (lib->job[slot].planned.directed) {  // owner-directed exchange: a rank holds the runs of its own videos' pairs, nothing else
    Job &j = const_cast<NeedleHipLibrary *>(lib)->job[slot];
    Status s = fetch_directed(j);
    if (!s.ok()) return report(s);
    *runs = j.found.fetched.data();
    *num_runs = j.found.fetched.size();
    return NeedleError_Ok;
  }
  const Job::Found &found = lib->job[slot].found;
  if (!found.last_runs && found.last_total) return NeedleError_InvalidArgument;
  *runs = found.last_runs;
  *num_runs = found.last_total;
  return NeedleError_Ok;
}

enum NeedleError needle_hip_library_job_form(const NeedleHipLibrary *lib, int slot, uint32_t form[4]) {
  if (!lib || !form) return NeedleError_NullArgument;
  if (slot < 0 || slot > 1 || lib->job[slot].pending) return NeedleError_InvalidArgument;
  const Job &j = lib->job[slot];
  form[0] = j.found.ran_device_epilogue ? 1u : 0u;
  form[1] = j.found.ran_sharded ? 1u : 0u;
  form[2] = j.planned.directed ? 1u : 0u;
  form[3] = j.planned.scan_form;
  return NeedleError_Ok;
}

enum NeedleError needle_hip_library_job_comm_bytes(const NeedleHipLibrary *lib, int slot, uint64_t bytes[4]) {
  if (!lib || !bytes) return NeedleError_NullArgument;
  if (slot < 0 || slot > 1) return NeedleError_InvalidArgument;
  std::copy(lib->job[slot].found.comm_bytes, lib->job[slot].found.comm_bytes + 4, bytes);
  return NeedleError_Ok;
}

int needle_hip_host_threads(void) { return (int)host_threads(); }

enum NeedleError needle_hip_library_audit(NeedleHipLibrary *lib, NeedleHipCertAudit *audit) {
  if (!lib || !audit) return NeedleError_NullArgument;
  if (!lib->have_pcm || !lib->pcm_resident) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    std::vector<StreamSpan> spans;
    Status s = block_spans(lib, comm_world(), comm_rank(), &spans);
    if (!s.ok()) return report(s);
    uint64_t c[4] = {0, 0, 0, 0};
    *audit = NeedleHipCertAudit{};
    if (spans.empty()) return NeedleError_Ok;
    s = gpu_fingerprint_audit_device(lib->d_pcm.ptr, spans, lib->channels, lib->step, lib->arena, c, &audit->max_error_over_s,
                                     &audit->max_s);
    if (!s.ok()) return report(s);
    audit->items = c[0];
    audit->accepted = c[1];
    audit->accepted_mismatches = c[2];
    audit->mismatches = c[3];
    return NeedleError_Ok;
  });
}

}  // extern "C"
