// Shared host-side declarations for libneedle_capi.so (MI355X-native needle analyze/search path).
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/needle_hip.h"

struct ihipStream_t;  // hipStream_t = ihipStream_t * (hip_runtime_api.h), without pulling HIP into host-only files

namespace needle {

// ---- errors -------------------------------------------------------------------------------------------
// Mirrors needle::Error (needle/src/lib.rs:117-149) closely enough to reproduce the mapping to
// NeedleError done in needle-capi/src/lib.rs:121-134.
struct Status {
  NeedleError code = NeedleError_Ok;
  std::string message;
  bool ok() const { return code == NeedleError_Ok; }
  static Status Ok() { return Status{}; }
  static Status Make(NeedleError c, std::string m) { return Status{c, std::move(m)}; }
};

// Records the message for needle_hip_last_error_message() and, like lib.rs:124, prints
// "needle error: ..." on stderr; returns the code.
NeedleError report(const Status &s);
void set_last_error(const std::string &m);
const char *last_error();

// ---- std::time::Duration, kept as total nanoseconds ----------------------------------------------------
using ns_t = uint64_t;
constexpr ns_t kNanosPerSec = 1000000000ull;

ns_t duration_from_secs_f32(float s, bool *ok = nullptr);   // Duration::from_secs_f32 (round to nearest ns, ties even)
ns_t duration_from_secs_f64(double s, bool *ok = nullptr);  // Duration::from_secs_f64
float duration_as_secs_f32(ns_t d);                         // Duration::as_secs_f32
double duration_as_secs_f64(ns_t d);
ns_t duration_mul_f32(ns_t d, float rhs, bool *ok = nullptr);  // Duration::mul_f32

// ---- FrameHashes (needle/src/audio/data.rs:15-26,74-80) -------------------------------------------------
struct HashTs {
  uint32_t hash;
  ns_t ts;
};

struct FrameHashesData {
  std::vector<HashTs> opening;
  std::vector<HashTs> ending;
  ns_t hash_duration = 0;
  std::string md5;
};

Status frame_hashes_read(const std::string &path, FrameHashesData *out);         // data.rs:104-115
Status frame_hashes_write(const std::string &path, const FrameHashesData &fh);   // analyzer.rs:414-417
Status header_md5(const std::string &path, std::string *out);                    // util.rs:99-105
std::string md5_hex(const uint8_t *data, size_t n);
std::string with_extension(const std::string &path, const std::string &ext);     // Path::with_extension
std::string format_time(ns_t t);                                                  // util.rs:8-12
std::string format_f32_json(float v);                                             // serde_json/ryu f32

// Host CPUs this process may use: hardware threads capped by its affinity mask and by the cgroup CPU quota (a
// container can see every core of the machine and be granted a few CPUs of time).
unsigned usable_cpus();
// This process's share of them: usable_cpus() divided by the rank processes of this node (set_node_ranks(), called by
// the communicator with max(world, LOCAL_WORLD_SIZE); 1 without a communicator), at least 1.  Eight ranks on a 16-CPU
// share get two epilogue threads each instead of 8 x 16 threads on 16 CPUs.  NEEDLE_HOST_THREADS overrides it.
unsigned host_threads();
void set_node_ranks(unsigned ranks);

// ---- chromaprint-facing constants -------------------------------------------------
constexpr int kSampleRate = 11025;
constexpr int kFrameSize = 4096;
constexpr int kHop = 1365;
constexpr int kBands = 12;
constexpr int kFirTaps = 5;
constexpr int kMaxFilterWidth = 16;
constexpr int kItemLatency = (kFirTaps - 1) + (kMaxFilterWidth - 1);  // frames - items
constexpr int kDelayMs = 2600;        // chromaprint_get_delay_ms
constexpr int kItemDurationMs = 123;  // chromaprint_get_item_duration_ms

inline size_t num_frames(size_t samples) { return samples < (size_t)kFrameSize ? 0 : (samples - kFrameSize) / kHop + 1; }
inline size_t num_items(size_t samples) {
  size_t f = num_frames(samples);
  return f > (size_t)kItemLatency ? f - kItemLatency : 0;
}
inline size_t num_kept(size_t samples, uint32_t step) {
  size_t n = num_items(samples);
  return step ? (n + step - 1) / step : 0;
}

// analyzer.rs:293-318: timestamps of the kept items.  Returns false if step_by would be 0.
bool step_for_hash_duration(ns_t hash_duration, uint32_t *step);
void attach_timestamps(const uint32_t *kept, size_t n_kept, uint32_t step, bool has_seek, ns_t seek_to,
                       std::vector<HashTs> *out);

// ---- WAV (the only container this build decodes; FFmpeg is out of scope) ---------------------------------
struct WavData {
  int channels = 0;
  int sample_rate = 0;
  std::vector<int16_t> pcm;  // interleaved
};
Status wav_read(const std::string &path, WavData *out);  // the whole data chunk
struct WavInfo {
  int channels = 0, sample_rate = 0;
  int format = 0, bits = 0;  // 1 = integer PCM, 3 = IEEE float
  uint32_t channel_mask = 0; // dwChannelMask of a WAVE_FORMAT_EXTENSIBLE header, 0 otherwise
  uint64_t data_offset = 0;  // byte offset of the first sample in the file
  uint64_t frames = 0;       // samples per channel in the data chunk
};
Status wav_probe(const std::string &path, WavInfo *out);  // reads chunk headers only
// frames [first, first+count) as interleaved s16 (count * channels values)
Status wav_read_frames(const std::string &path, const WavInfo &info, uint64_t first, uint64_t count, int16_t *dst);

// ---- GPU entry points used by the host classes (fingerprint.hip, fingerprint_host.hip / search.hip) ----------------------------
struct StreamSpan {
  uint64_t pcm_off;     // offset into the PCM arena, in s16 values
  uint64_t num_values;  // interleaved values
  uint64_t item_off;    // offset into the item arena where kept items go
};

Status gpu_fingerprint_device(const int16_t *d_pcm, const std::vector<StreamSpan> &streams, int channels,
                              uint32_t step, uint32_t *d_items, bool sync, double *d_chroma_dbg = nullptr,
                              double *d_feat_dbg = nullptr, size_t descriptor_slot = 0, int pipe = -1,
                              uint32_t *zero_word = nullptr, bool *zeroed = nullptr);
// (zero_word: a device word the caller wants cleared behind the fingerprinting -- the run counter of the scan that
// follows -- by the last kernel of the call instead of a memset dispatch; *zeroed says whether that happened.)
// (pipe 0 / 1: the caller keeps two calls in flight, e.g. the two job slots of a library.  The f32 STFT of such a call
// runs on the CU-masked stream of hipctx.hip into workspace `pipe`, so that it overlaps whatever the previous call still
// has queued on the library stream; everything behind it stays on the library stream.  -1: everything on the library
// stream, one workspace.)
// Host PCM -> kept items in DEVICE memory (d_items + item_off[i]), uploads and kernels overlapped: the streams are
// uploaded in order on the upload stream and fingerprinted group by group (about NEEDLE_HIP_LAUNCH_GROUP_BYTES of
// PCM each) on the library stream as they land.  The PCM is not kept.  On return every copy out of host memory has
// executed; the kernels may still be running (library stream order).
Status gpu_fingerprint_streamed_device(const std::vector<const int16_t *> &pcm, const std::vector<size_t> &num_values,
                                       int channels, uint32_t step, uint32_t *d_items,
                                       const std::vector<uint64_t> &item_off, int rate = kSampleRate);
// `rate` != 11025 routes the streams through the device resampler first (resample.hip).
Status gpu_fingerprint_host(const std::vector<const int16_t *> &pcm, const std::vector<size_t> &num_values,
                            int channels, uint32_t step, std::vector<std::vector<uint32_t>> *items,
                            int rate = kSampleRate);
// Same with the PCM produced by `read` (stream index, first value, value count -> interleaved s16 at dst, which is
// pinned host memory): up to `readers` threads call it concurrently for different segments while earlier segments
// are on their way to the device.  Host memory stays a fixed ring of slabs whatever the streams' lengths.
using PcmReader = std::function<Status(size_t stream, uint64_t first_value, uint64_t num_values, int16_t *dst)>;
// The upload alone (hipctx.hip): stream i goes to d_pcm + dev_off[i] (offsets in values, multiples of 8), copied on
// `stream` (NULL: the library stream).  On return the copies have executed.  `issued` (optional) is called on the
// issuing thread right after the last copy of a stream has been enqueued, streams in order (zero-length streams of
// the ring path are skipped): the caller's place to queue work behind an event of `stream`.
using StreamIssued = std::function<Status(size_t stream_index)>;
Status gpu_upload_pcm_streamed(const std::vector<size_t> &num_values, const std::vector<uint64_t> &dev_off,
                               const PcmReader &read, unsigned readers, int16_t *d_pcm, ::ihipStream_t *stream = nullptr,
                               const StreamIssued &issued = nullptr);
// Same from host pointers.  Pinned host memory is copied in place and small totals go as plain asynchronous copies
// (in both cases nothing need have executed on return, as with hipMemcpyAsync); large pageable totals go through the ring.
Status gpu_upload_pcm(const std::vector<const int16_t *> &pcm, const std::vector<size_t> &num_values,
                      const std::vector<uint64_t> &dev_off, int16_t *d_pcm, ::ihipStream_t *stream = nullptr,
                      const StreamIssued &issued = nullptr);
Status gpu_fingerprint_streamed(const std::vector<size_t> &num_values, const PcmReader &read, unsigned readers,
                                int channels, uint32_t step, std::vector<std::vector<uint32_t>> *items,
                                int rate = kSampleRate, const NeedleHipChannelMix *mix = nullptr);
Status gpu_hamming_runs_device(const uint32_t *d_hashes, const NeedleHipSeq *seqs, size_t num_seqs,
                               const NeedleHipProblem *problems, size_t num_problems, uint32_t threshold,
                               NeedleHipRun *d_runs, uint32_t capacity, uint32_t *d_count, bool sync,
                               bool count_is_zero = false);
Status gpu_hamming_runs_host(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *seqs, size_t num_seqs,
                             const NeedleHipProblem *problems, size_t num_problems, uint32_t threshold,
                             std::vector<NeedleHipRun> *runs);

// the hash arena of a search call in pinned host memory, and its upload enqueued ahead of the call (search.hip)
uint32_t *gpu_pinned_arena_acquire(size_t words);  // nullptr: none to be had (no device, or one is handed out already)
void gpu_pinned_arena_release(uint32_t *arena);
void gpu_prefetch_hashes(const uint32_t *hashes, size_t num_hashes);

// Sequence pairs from which the per-video epilogue runs on the device (epilogue.hip) instead of on host threads
// (NEEDLE_HIP_DEVICE_EPILOGUE=1 / 0 forces either): the library job and Comparator::run_with_frame_hashes alike.
constexpr uint64_t kDeviceEpiloguePairs = 1u << 14;
constexpr uint32_t kDeviceEpilogueRuns = 1u << 14;  // ... or from this many runs per rank in the library's last finished job

// Diagnostic (search.hip): cells/s of the band scan's 4-instruction cell on registers only, measured on this device.
Status gpu_int_valu_ceiling(double *cells_per_second);
Status gpu_scan_issued_evaluations(uint64_t *lane_evaluations, bool reset, uint64_t *head_survivors = nullptr);
void gpu_scan_last_launch(int32_t *form, uint64_t *matrix_products);  // needle_hip_scan_last_launch
// certified f32 first pass of the fingerprinter: {items, items recomputed in f64, chunks of frame pairs, chunks recomputed}
Status gpu_fingerprint_cert_stats(uint64_t out[4], bool reset);
// audit of that first pass: both transforms over the same PCM, every kept item compared on the device (fingerprint.hip)
Status gpu_fingerprint_audit_device(const int16_t *d_pcm, const std::vector<StreamSpan> &spans, int channels, uint32_t step,
                                    const uint32_t *d_items, uint64_t out[4], double *max_ratio, double *max_sigma);

// One lane's share of a feed of the streaming fingerprinter (feeder.hip -> fingerprint.hip): where its PCM tail and its
// chroma / energy rows lie in the feeder's buffers.  Rows [0, carried) hold first-pass rows of earlier feeds, rows
// [carried, frames) are transformed now; `kept` new items, the first of them `first_item` rows in.
struct FeedLane {
  uint64_t pcm_off;     // s16 values: frame 0 of the lane's rows starts here
  uint64_t item_off;    // where the new kept items go in d_items
  uint32_t row_base;    // the lane's first chroma / energy row
  uint32_t carried;     // even
  uint32_t frames;      // carried + new
  uint32_t first_item;
  uint32_t kept;
  uint32_t lane;        // the feeder's lane: where an audited feed counts this stream's items
};
// An audited feed (needle_hip_feeder_set_audit): behind everything a feed runs, the f64 kernel over the NEW frame pairs
// into `rows64` -- rows the audit owns, numbered like d_chroma, the carried ones already there -- and audit_items_kernel
// over carried + new, every new kept item counted into counts[lane] (kFeedAuditWords words per lane, resident).
constexpr size_t kFeedAuditWords = 6;  // {items, accepted, accepted wrong, final wrong, max ratio bits, max sigma bits}
struct FeedAudit {
  double *rows64;
  uint64_t *counts;
};
Status gpu_fingerprint_feed_device(const int16_t *d_pcm, const std::vector<FeedLane> &lanes, int channels, uint32_t step,
                                   double *d_chroma, float *d_energy, double *d_chroma64, uint32_t *d_items,
                                   const FeedAudit *audit = nullptr);
bool gpu_fingerprint_f64_mode();  // NEEDLE_HIP_STFT=f64: no first pass, nothing to audit
// test hook: the certified chain of gpu_fingerprint_device over host PCM, with what each kernel wrote (needle_hip.h)
Status gpu_fingerprint_stages_debug(const std::vector<const int16_t *> &pcm, const std::vector<size_t> &num_values, int channels,
                                    uint32_t step, uint32_t flags, NeedleHipStages *out);

// ---- resampler front-end (resample.hip) -------------------------------------------------------------------
struct ResampleSpan {
  uint64_t in_off;   // offset into the input arena, in s16 values
  uint64_t n_in;     // samples per channel: the stream's true extent [0, n_in), zeros outside it
  uint64_t out_off;  // offset into the output arena, in samples (of the stream's output 0)
  // Optional, for streams that are not whole streams of the input arena:
  //  * src: the stream's own source (any 2-byte alignment) instead of d_in + in_off.  With a piece, src points at
  //    sample p0 (the piece's first), not at sample 0.
  //  * tiles [t0, t1): only those output tiles (resample_tiling().tile_outputs each) are computed; t1 == 0: to the end.
  //  * piece [p0, p1): the input samples that are there to be read (p1 == 0: the whole stream).  It must cover the taps
  //    of the tiles' outputs (resample_piece); its edges are not the stream's, zeros come only from outside [0, n_in).
  // The output is bit for bit the same slice of the whole stream's output.
  // (out_off is taken modulo 2^64: with tiles, only the places of the outputs computed need lie in the arena -- the
  // streaming feeder keeps a stream's tail alone, and its output 0 then lies in front of the arena.)
  const int16_t *src = nullptr;
  uint64_t t0 = 0, t1 = 0;
  uint64_t p0 = 0, p1 = 0;
};
size_t resample_out_len(size_t n_in, int rate);
// The kernel gpu_resample_device picks for `rate` (environment overrides included) computes whole tiles of
// tile_outputs consecutive outputs; output m reads input samples [m M / L - half + 1, m M / L + half + 1) (floor).
struct ResampleTiling {
  int L = 1, M = 1, half = 0;
  uint64_t tile_outputs = 1;
};
Status resample_tiling(int rate, int channels, ResampleTiling *out);
// the same without a device (the kernel's choice and its tiles are host arithmetic on the rate)
Status resample_tiling_host(int rate, ResampleTiling *out);
// the whole plan of `rate` as the launch reads it, for needle_hip_resample_plan; no device, no coefficients
Status resample_plan_host(int rate, NeedleHipResamplePlan *out);
// the input samples [*p0, *p1) of a stream of n_in samples that tiles [t0, t1) read, p0 rounded down to a multiple of 8
void resample_piece(const ResampleTiling &t, uint64_t n_in, uint64_t t0, uint64_t t1, uint64_t *p0, uint64_t *p1);
Status gpu_resample_device(const int16_t *d_in, const std::vector<ResampleSpan> &spans, int channels, int rate,
                           int16_t *d_out, bool sync);
Status gpu_resample_host(const std::vector<const int16_t *> &pcm, const std::vector<size_t> &num_values, int channels,
                         int rate, std::vector<std::vector<int16_t>> *out);

// ---- down-mix of 3-8 channel PCM (downmix.hip) -------------------------------------------------------------
// mono[n] = (sum of the C values of frame n) / C, C integer division; a trailing partial frame is dropped.
struct DownmixSpan {
  const int16_t *src;  // interleaved C-channel frames (device); any 2-byte alignment
  int16_t *dst;        // mono (device), a buffer of its own
  uint64_t frames;
};
// one launch on the library stream for all spans; returns after enqueueing unless `sync`
Status gpu_downmix_device(const std::vector<DownmixSpan> &spans, int channels, bool sync);
// host arrays in and out (out[i] holds num_values[i] / channels values), in batches of bounded device memory
Status gpu_downmix_host(const std::vector<const int16_t *> &pcm, const std::vector<size_t> &num_values, int channels,
                        const std::vector<int16_t *> &out);

// ---- sample formats (convert.hip): NeedleHipSampleFormat -> s16, on the device ------------------------------
inline bool sample_format_valid(int format) { return format >= NEEDLE_HIP_SAMPLE_U8 && format <= NEEDLE_HIP_SAMPLE_F64P; }
inline bool sample_format_planar(int format) { return format >= NEEDLE_HIP_SAMPLE_U8P; }
inline size_t sample_format_width(int format) {  // bytes per sample
  constexpr size_t width[5] = {1, 2, 4, 4, 8};
  return width[format % 5];
}
// pointers a caller passes per stream: one per channel when planar
inline size_t sample_format_planes(int format, int channels) { return sample_format_planar(format) ? (size_t)channels : 1; }
// s16 units (2 bytes) a plane -- or an interleaved stream -- of `samples` samples takes in a raw staging arena: every
// plane starts 16-byte aligned there (the kernel's vector path)
inline uint64_t sample_plane_units(uint64_t samples, size_t width) { return ((samples * width + 15) & ~(uint64_t)15) / 2; }
struct ConvertSpan {
  const void *src[NEEDLE_HIP_MAX_CHANNELS];  // device; planar: plane c (frames samples each), interleaved: src[0] (frames * C
                                             // samples).  Aligned to one sample at least.
  int16_t *dst;                              // device, a buffer of its own: frames * C interleaved values, or frames mono ones
  uint64_t frames;
};
// One launch on the library stream for all spans; returns after enqueueing unless `sync`.  `mix` (3-8 channels): the
// down-mix of downmix.hip fused in, mono out; otherwise interleaved `channels`-channel s16 out.
Status gpu_convert_device(const std::vector<ConvertSpan> &spans, int channels, int format, bool mix, bool sync);
// Raw samples of any width from host pointers: stream i (bytes[i] bytes) goes to d_raw + dev_off[i] (offsets in s16
// units, multiples of 8); otherwise as gpu_upload_pcm.
Status gpu_upload_raw(const std::vector<const void *> &src, const std::vector<size_t> &bytes, const std::vector<uint64_t> &dev_off,
                      int16_t *d_raw, ::ihipStream_t *stream = nullptr, const StreamIssued &issued = nullptr);
// gpu_fingerprint_host / gpu_fingerprint_streamed_device with the streams in `format` (fingerprint_host.hip): uploaded as
// they are, converted on the device group by group under the uploads.  pcm: sample_format_planes() pointers per stream.
Status gpu_fingerprint_host_format(const std::vector<const void *> &pcm, const std::vector<size_t> &num_values, int channels,
                                   int format, uint32_t step, std::vector<std::vector<uint32_t>> *items, int rate = kSampleRate,
                                   const NeedleHipChannelMix *mix = nullptr);
Status gpu_fingerprint_streamed_device_format(const std::vector<const void *> &pcm, const std::vector<size_t> &num_values,
                                              int channels, int format, uint32_t step, uint32_t *d_items,
                                              const std::vector<uint64_t> &item_off, int rate = kSampleRate,
                                              const NeedleHipChannelMix *mix = nullptr);
// (`mix`, in the three above: a channel mix -- the streams of any format and channel count are landed as mono by
// rematrix.hip, group by group under the uploads, and go on as mono s16)
// host arrays in and out (pcm: sample_format_planes() pointers per stream; out[i] holds num_values[i] / channels * channels
// interleaved s16 values, not down-mixed), in batches of bounded device memory
Status gpu_convert_host(const std::vector<const void *> &pcm, const std::vector<size_t> &num_values, int channels, int format,
                        const std::vector<int16_t *> &out);

// ---- the front end of a feeder whose lanes have formats of their own (convert.hip feeder_ingest_kernel) -----
// A span in its own format -> mono s16: gpu_convert_host's conversion, then gpu_downmix_host's (sum of the frame's
// `channels` converted values) / channels, whatever the channel count (1: the conversion alone).
struct IngestSpan {
  const void *src[NEEDLE_HIP_MAX_CHANNELS];  // device; as ConvertSpan's, by the span's own format and channels
  int16_t *dst;                              // device, a buffer of its own: frames mono values, any 2-byte alignment
  uint64_t frames;
  int channels, format;
  const NeedleHipChannelMix *mix = nullptr;  // gpu_rematrix_device only; nullptr: the plain average
};
// one launch on the library stream for all spans, whatever mixture of formats; returns after enqueueing unless `sync`
Status gpu_ingest_device(const std::vector<IngestSpan> &spans, bool sync);
// host arrays in and out (pcm: the concatenation of every stream's sample_format_planes() pointers; out[i] holds
// num_values[i] / channels[i] values), in batches of bounded device memory
Status gpu_convert_mono_host(const std::vector<const void *> &pcm, const std::vector<size_t> &num_values,
                             const std::vector<int> &channels, const std::vector<int> &formats, const std::vector<int16_t *> &out,
                             const NeedleHipChannelMix *mixes = nullptr);

// ---- channel mixes: the layout-aware fold-down to stereo, then mono (rematrix.hip; needle_hip.h has the arithmetic) --
// the limits of a mix, and that it is one for `channels` channels; host arithmetic (hostutil.cpp)
Status channel_mix_check(const NeedleHipChannelMix &mix, int channels);
Status channel_mix_default(uint32_t channel_mask, NeedleHipChannelMix *out);
// gpu_ingest_device with a mix per span: one launch of rematrix_kernel on the library stream for all spans, those
// without a mix through the shared ingest_block.  gpu_convert_mono_host with `mixes` (one per stream, channels == 0:
// none) runs this instead of gpu_ingest_device.
Status gpu_rematrix_device(const std::vector<IngestSpan> &spans, bool sync);

}  // namespace needle
