// Host PCM -> kept items: plans device batches over the streams, uploads them and runs the (converter, down-mix,
// resampler and) fingerprinter group by group underneath the copies that follow.  Nothing here launches a kernel of its
// own: it calls gpu_fingerprint_device and friends (common.h).
#include "format_plan.h"
#include "hipctx.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>

namespace needle {

namespace {

// Per device, kept for the life of the process like the other workspaces (never destroyed: HIP may already be
// gone when static destructors run).  The arenas grow to the largest batch seen (at most 2 GiB of PCM).
struct HostEntryWorkspace {
  DeviceBuffer<int16_t> d_pcm, d_mono;
  DeviceBuffer<int16_t> d_mixed;  // 3-8 channel input down-mixed to mono (what the resampler or fingerprinter then reads)
  DeviceBuffer<int16_t> d_raw;    // samples in another format than s16, as uploaded (what the conversion reads)
  DeviceBuffer<uint32_t> d_items;
};

HostEntryWorkspace *host_entry_workspace() {
  static std::mutex mu;
  static std::map<int, HostEntryWorkspace *> all;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  HostEntryWorkspace *&w = all[dev];
  if (!w) w = new HostEntryWorkspace();
  return w;
}

// Plans device batches over the streams and, inside a batch, overlaps the host -> device copies with the kernels:
// `upload` copies the batch's streams in order on the upload stream and reports each stream as its last copy is
// enqueued; every time about `group_bytes` of PCM have been enqueued, an event is recorded behind them and the
// (resampler +) fingerprinter of those streams is launched on the library stream behind that event.  The copy
// engine therefore never waits for kernels and the kernels of all but the last group are hidden under the copies
// that follow.  Items go to the host (`items`) or stay on the device (`d_items_out` + `item_off_out`).
using BatchUpload = std::function<Status(size_t begin, size_t end, const std::vector<uint64_t> &in_off, int16_t *d_pcm,
                                         hipStream_t stream, const StreamIssued &issued)>;

struct OverlapEvents {  // per device, reused by every call (guarded by gpu_mutex())
  hipEvent_t landed = nullptr, batch_done = nullptr, entry = nullptr;
};
OverlapEvents *overlap_events() {
  static std::mutex mu;
  static std::map<int, OverlapEvents *> all;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  OverlapEvents *&e = all[dev];
  if (!e) {
    e = new OverlapEvents();
    (void)hipEventCreateWithFlags(&e->landed, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&e->batch_done, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&e->entry, hipEventDisableTiming);
  }
  return e;
}

Status fingerprint_in_batches(const std::vector<size_t> &num_values, int channels, uint32_t step,
                              std::vector<std::vector<uint32_t>> *items, int rate, int format, const BatchUpload &upload,
                              uint32_t *d_items_out = nullptr, const std::vector<uint64_t> *item_off_out = nullptr,
                              const NeedleHipChannelMix *remix = nullptr) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s;
  if (remix && !(s = channel_mix_check(*remix, channels)).ok()) return s;  // before any device is asked for
  if (!(s = ensure_device()).ok()) return s;
  if (channels < 1 || channels > NEEDLE_HIP_MAX_CHANNELS)
    return Status::Make(NeedleError_InvalidArgument, "fingerprint: channels must be 1 to " + std::to_string(NEEDLE_HIP_MAX_CHANNELS));
  if (step == 0) return Status::Make(NeedleError_InvalidArgument, "fingerprint: step must be >= 1");
  const bool resample = rate != kSampleRate;
  // 3-8 channels: each launch group is down-mixed into d_mixed first and goes on as mono (downmix -> resample ->
  // fingerprint, the oracle's order); 1 and 2 channels are read by the resampler / STFT kernels themselves
  // Another sample format than interleaved s16: the streams are uploaded as they are into d_raw (`upload` is handed
  // that arena and the streams' offsets in it) and each launch group is converted into d_pcm first (convert.hip; 3-8
  // channels with the down-mix fused in), where the s16 path would have found them
  // A channel mix (`remix`): the streams go the same way whatever their format and channel count, s16 and 1-2 channels
  // included, and rematrix.hip lands each launch group in d_pcm as mono
  if (!sample_format_valid(format)) return Status::Make(NeedleError_InvalidArgument, "fingerprint: unknown sample format");
  const bool conv = format != NEEDLE_HIP_SAMPLE_S16 || remix;
  const int pcm_channels = conv && (channels > 2 || remix) ? 1 : channels;  // of what d_pcm holds
  const bool mix = !conv && channels > 2;
  const size_t planes = sample_format_planes(format, channels), width = sample_format_width(format);
  const size_t n = num_values.size();
  if (items) items->assign(n, {});
  // Batches bounded by bytes so the device arena stays modest for huge libraries.
  bool count_values = false;
  const uint64_t kMaxBatchValues = batch_limit(&count_values);  // 2 GiB of s16 (of raw samples, counted in s16 units, in another format)
  uint64_t group_values = (32ull << 20) / sizeof(int16_t);
  if (const char *e = getenv("NEEDLE_HIP_LAUNCH_GROUP_BYTES")) group_values = (uint64_t)std::max(2ll, atoll(e)) / sizeof(int16_t);
  hipStream_t stream = library_stream(), up = upload_stream();
  // Every exit of this function -- the error returns included -- waits for the copies already enqueued: they read the
  // caller's (pinned) buffers and the slab ring asynchronously, and the contract is that those are free on return.
  struct DrainUploads {
    hipStream_t s;
    ~DrainUploads() { (void)hipStreamSynchronize(s); }
  } drain_uploads{up};
  OverlapEvents *ev = overlap_events();
  HostEntryWorkspace *ws = host_entry_workspace();  // grow-only arenas, guarded by gpu_mutex()
  DeviceBuffer<int16_t> &d_pcm = ws->d_pcm, &d_mono = ws->d_mono, &d_mixed = ws->d_mixed, &d_raw = ws->d_raw;
  DeviceBuffer<uint32_t> &d_items = ws->d_items;
  size_t begin = 0, descriptor_slot = 0;
  bool first_batch = true;
  while (begin < n) {
    std::vector<StreamSpan> spans;        // what the fingerprinter reads (11025 Hz; mono if resampled)
    std::vector<ResampleSpan> rspans;     // what the resampler reads, when the input rate differs
    std::vector<ResampleSpan> mspans;     // what the down-mix reads and writes: (in_off, frames, offset in d_mixed)
    std::vector<ResampleSpan> cspans;     // what the conversion reads and writes: (offset in d_raw, frames, offset in d_pcm)
    std::vector<uint64_t> in_off;
    uint64_t values = 0, mono = 0, mixed = 0, kept = 0, raw = 0, raw_cost = 0;
    size_t end = begin;
    while (end < n) {
      const size_t in_samples = num_values[end] / (size_t)channels;
      const uint64_t pcm_values = conv ? (uint64_t)in_samples * pcm_channels : num_values[end];  // of the stream in d_pcm
      const uint64_t raw_units = conv ? planes * sample_plane_units(in_samples * (planes == 1 ? channels : 1), width) : 0;
      const uint64_t cost = conv && !count_values ? raw_units : num_values[end];
      if (!spans.empty() && (conv ? raw_cost : values) + cost > kMaxBatchValues) break;
      const size_t out_samples = resample ? resample_out_len(in_samples, rate) : in_samples;
      const uint64_t item_off = d_items_out ? (*item_off_out)[end] : kept;
      in_off.push_back(conv ? raw : values);
      if (conv) cspans.push_back(ResampleSpan{raw, in_samples, values});
      raw += raw_units;
      raw_cost += cost;
      uint64_t src_off = values;  // where the resampler or the fingerprinter reads this stream
      if (mix) {
        mspans.push_back(ResampleSpan{values, in_samples, mixed});
        src_off = mixed;
        mixed += (in_samples + 7) & ~(uint64_t)7;  // 16-byte aligned, as the arena's streams
      }
      if (resample) {
        rspans.push_back(ResampleSpan{src_off, in_samples, mono});
        spans.push_back(StreamSpan{mono, out_samples, item_off});
        mono += (out_samples + 1) & ~(uint64_t)1;
      } else {
        spans.push_back(StreamSpan{src_off, mix ? in_samples : pcm_values, item_off});
      }
      values += (pcm_values + 7) & ~(uint64_t)7;  // keep every stream 16-byte aligned in the arena
      kept += num_kept(out_samples, step);
      end++;
    }
    const bool trace = getenv("NEEDLE_HIP_TRACE") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
      if (!trace) return;
      const auto now = std::chrono::steady_clock::now();
      std::fprintf(stderr, "[needle_hip] fingerprint_host %s: %.2f ms\n", what,
                   std::chrono::duration<double, std::milli>(now - t0).count());
      t0 = now;
    };
    if (!(s = d_pcm.reserve(std::max<uint64_t>(values, 1))).ok()) return s;
    if (!d_items_out && !(s = d_items.reserve(std::max<uint64_t>(kept, 1))).ok()) return s;
    if (resample && !(s = d_mono.reserve(std::max<uint64_t>(mono, 1))).ok()) return s;
    if (mix && !(s = d_mixed.reserve(std::max<uint64_t>(mixed, 1))).ok()) return s;
    if (conv && !(s = d_raw.reserve(std::max<uint64_t>(raw, 1))).ok()) return s;
    uint32_t *const d_out = d_items_out ? d_items_out : d_items.ptr;
    lap("device allocations");
    // the copies must not overtake kernels that still read the PCM arena: those of the previous batch, or of an
    // earlier call on the library stream
    NEEDLE_HIP_TRY(hipEventRecord(first_batch ? ev->entry : ev->batch_done, stream));
    NEEDLE_HIP_TRY(hipStreamWaitEvent(up, first_batch ? ev->entry : ev->batch_done, 0));
    first_batch = false;
    size_t launched = 0;       // streams of this batch whose kernels have been enqueued
    uint64_t pending_values = 0;
    auto launch_group = [&](size_t upto) -> Status {  // streams [launched, upto) of the batch have been enqueued on `up`
      if (upto <= launched) return Status::Ok();
      NEEDLE_HIP_TRY(hipEventRecord(ev->landed, up));
      NEEDLE_HIP_TRY(hipStreamWaitEvent(stream, ev->landed, 0));
      const std::vector<StreamSpan> group(spans.begin() + launched, spans.begin() + upto);
      Status gs;
      const int16_t *src = d_pcm.ptr;
      int src_channels = pcm_channels;
      if (conv) {  // raw samples -> s16 (3-8 channels: mono), into d_pcm (behind the same event as the kernels it feeds)
        std::vector<ConvertSpan> cgroup;
        std::vector<IngestSpan> rgroup;
        for (size_t k = launched; k < upto; k++) {
          ConvertSpan sp{};
          const uint64_t plane = sample_plane_units(cspans[k].n_in * (planes == 1 ? channels : 1), width);
          for (size_t c = 0; c < planes; c++) sp.src[c] = d_raw.ptr + cspans[k].in_off + c * plane;
          sp.dst = d_pcm.ptr + cspans[k].out_off;
          sp.frames = cspans[k].n_in;
          cgroup.push_back(sp);
          if (remix) {
            IngestSpan in{};
            std::memcpy(in.src, sp.src, sizeof(in.src));
            in.dst = sp.dst;
            in.frames = sp.frames;
            in.channels = channels;
            in.format = format;
            in.mix = remix;
            rgroup.push_back(in);
          }
        }
        gs = remix ? gpu_rematrix_device(rgroup, false) : gpu_convert_device(cgroup, channels, format, channels > 2, false);
      }
      if (mix) {  // C-channel PCM -> mono, into d_mixed (behind the same event as the kernels it feeds)
        std::vector<DownmixSpan> mgroup;
        for (size_t k = launched; k < upto; k++)
          mgroup.push_back(DownmixSpan{d_pcm.ptr + mspans[k].in_off, d_mixed.ptr + mspans[k].out_off, mspans[k].n_in});
        gs = gpu_downmix_device(mgroup, channels, false);
        src = d_mixed.ptr;
        src_channels = 1;
      }
      if (gs.ok() && resample) {  // decode-rate PCM -> mono 11025 Hz, on the device, then straight into the fingerprinter
        const std::vector<ResampleSpan> rgroup(rspans.begin() + launched, rspans.begin() + upto);
        gs = gpu_resample_device(src, rgroup, src_channels, rate, d_mono.ptr, false);
        src = d_mono.ptr;
        src_channels = 1;
      }
      if (gs.ok()) gs = gpu_fingerprint_device(src, group, src_channels, step, d_out, false, nullptr, nullptr, descriptor_slot++);
      launched = upto;
      pending_values = 0;
      return gs;
    };
    const StreamIssued issued = [&](size_t i) -> Status {  // i: index inside the batch
      pending_values += num_values[begin + i];
      if (pending_values >= group_values) return launch_group(i + 1);
      return Status::Ok();
    };
    if (!(s = upload(begin, end, in_off, conv ? d_raw.ptr : d_pcm.ptr, up, issued)).ok()) return s;
    if (!(s = launch_group(end - begin)).ok()) return s;
    lap("upload + kernel launches");
    if (items) {
      std::vector<uint32_t> host(std::max<uint64_t>(kept, 1));
      NEEDLE_HIP_TRY(hipMemcpyAsync(host.data(), d_items.ptr, kept * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
      for (size_t i = begin; i < end; i++) {
        const size_t in_samples = num_values[i] / (size_t)channels;
        const size_t k = num_kept(resample ? resample_out_len(in_samples, rate) : in_samples, step);
        (*items)[i].assign(host.begin() + spans[i - begin].item_off, host.begin() + spans[i - begin].item_off + k);
      }
      lap("download + scatter");
    }
    begin = end;
  }
  // every copy out of host memory has executed when this returns (the callers' buffers and the slab ring are free)
  NEEDLE_HIP_TRY(hipStreamSynchronize(up));
  return Status::Ok();  // (drain_uploads then finds the stream idle)
}

// the upload of interleaved s16 streams from host pointers
BatchUpload pcm_upload(const std::vector<const int16_t *> &pcm, const std::vector<size_t> &num_values) {
  return [&pcm, &num_values](size_t begin, size_t end, const std::vector<uint64_t> &in_off, int16_t *d_pcm, hipStream_t up,
                             const StreamIssued &issued) -> Status {
    return gpu_upload_pcm(std::vector<const int16_t *>(pcm.begin() + begin, pcm.begin() + end),
                          std::vector<size_t>(num_values.begin() + begin, num_values.begin() + end), in_off, d_pcm, up, issued);
  };
}

}  // namespace

Status gpu_fingerprint_host(const std::vector<const int16_t *> &pcm, const std::vector<size_t> &num_values,
                            int channels, uint32_t step, std::vector<std::vector<uint32_t>> *items, int rate) {
  if (pcm.size() != num_values.size())
    return Status::Make(NeedleError_InvalidArgument, "fingerprint: one length per stream is required");
  return fingerprint_in_batches(num_values, channels, step, items, rate, NEEDLE_HIP_SAMPLE_S16, pcm_upload(pcm, num_values));
}

Status gpu_fingerprint_streamed(const std::vector<size_t> &num_values, const PcmReader &read, unsigned readers,
                                int channels, uint32_t step, std::vector<std::vector<uint32_t>> *items, int rate,
                                const NeedleHipChannelMix *mix) {
  return fingerprint_in_batches(
      num_values, channels, step, items, rate, NEEDLE_HIP_SAMPLE_S16,
      [&](size_t begin, size_t end, const std::vector<uint64_t> &in_off, int16_t *d_pcm, hipStream_t up,
          const StreamIssued &issued) -> Status {
        const PcmReader shifted = [&](size_t stream, uint64_t first, uint64_t count, int16_t *dst) {
          return read(begin + stream, first, count, dst);
        };
        return gpu_upload_pcm_streamed(std::vector<size_t>(num_values.begin() + begin, num_values.begin() + end), in_off,
                                       shifted, readers, d_pcm, up, issued);
      },
      nullptr, nullptr, mix);
}

Status gpu_fingerprint_streamed_device(const std::vector<const int16_t *> &pcm, const std::vector<size_t> &num_values,
                                       int channels, uint32_t step, uint32_t *d_items,
                                       const std::vector<uint64_t> &item_off, int rate) {
  if (pcm.size() != num_values.size() || item_off.size() != num_values.size())
    return Status::Make(NeedleError_InvalidArgument, "fingerprint: one length and one item offset per stream are required");
  return fingerprint_in_batches(num_values, channels, step, nullptr, rate, NEEDLE_HIP_SAMPLE_S16, pcm_upload(pcm, num_values), d_items,
                                &item_off);
}

namespace {
// The upload of streams in another sample format than interleaved s16: every plane of a stream (one, if interleaved)
// goes to its 16-byte aligned place in the raw arena, and the stream is reported once its last plane is on its way.
BatchUpload raw_upload(const std::vector<const void *> &pcm, const std::vector<size_t> &num_values, int channels, int format) {
  return [&pcm, &num_values, channels, format](size_t begin, size_t end, const std::vector<uint64_t> &in_off, int16_t *d_raw,
                                               hipStream_t up, const StreamIssued &issued) -> Status {
    const size_t planes = sample_format_planes(format, channels), width = sample_format_width(format);
    std::vector<const void *> src;
    std::vector<size_t> bytes;
    std::vector<uint64_t> off;
    for (size_t i = begin; i < end; i++) {
      const uint64_t samples = num_values[i] / (size_t)channels * (planes == 1 ? (size_t)channels : 1);  // of one plane
      for (size_t c = 0; c < planes; c++) {
        src.push_back(pcm[i * planes + c]);
        bytes.push_back(samples * width);
        off.push_back(in_off[i - begin] + c * sample_plane_units(samples, width));
      }
    }
    const StreamIssued plane_issued = [&](size_t k) -> Status { return k % planes == planes - 1 ? issued(k / planes) : Status::Ok(); };
    return gpu_upload_raw(src, bytes, off, d_raw, up, plane_issued);
  };
}
}  // namespace

Status gpu_fingerprint_host_format(const std::vector<const void *> &pcm, const std::vector<size_t> &num_values, int channels,
                                   int format, uint32_t step, std::vector<std::vector<uint32_t>> *items, int rate,
                                   const NeedleHipChannelMix *mix) {
  if (!sample_format_valid(format) || channels < 1 || channels > NEEDLE_HIP_MAX_CHANNELS)
    return Status::Make(NeedleError_InvalidArgument, "fingerprint: unknown sample format or channel count");
  if (pcm.size() != num_values.size() * sample_format_planes(format, channels))
    return Status::Make(NeedleError_InvalidArgument, "fingerprint: one length per stream and one pointer per plane are required");
  if (format == NEEDLE_HIP_SAMPLE_S16 && !mix) {
    std::vector<const int16_t *> s16(pcm.size());
    for (size_t i = 0; i < pcm.size(); i++) s16[i] = static_cast<const int16_t *>(pcm[i]);
    return gpu_fingerprint_host(s16, num_values, channels, step, items, rate);
  }
  return fingerprint_in_batches(num_values, channels, step, items, rate, format, raw_upload(pcm, num_values, channels, format), nullptr,
                                nullptr, mix);
}

Status gpu_fingerprint_streamed_device_format(const std::vector<const void *> &pcm, const std::vector<size_t> &num_values,
                                              int channels, int format, uint32_t step, uint32_t *d_items,
                                              const std::vector<uint64_t> &item_off, int rate, const NeedleHipChannelMix *mix) {
  if (!sample_format_valid(format) || channels < 1 || channels > NEEDLE_HIP_MAX_CHANNELS)
    return Status::Make(NeedleError_InvalidArgument, "fingerprint: unknown sample format or channel count");
  if (pcm.size() != num_values.size() * sample_format_planes(format, channels) || item_off.size() != num_values.size())
    return Status::Make(NeedleError_InvalidArgument, "fingerprint: one length and one item offset per stream, one pointer per plane are required");
  return fingerprint_in_batches(num_values, channels, step, nullptr, rate, format, raw_upload(pcm, num_values, channels, format),
                                d_items, &item_off, mix);
}

// The plan of fingerprint_in_batches for streams with formats of their own.  Every stream goes on as mono: a batch's
// streams are uploaded raw into d_raw (every plane 16-byte aligned), a launch group is landed by one launch -- 11025 Hz
// streams straight into d_mono, where the fingerprinter reads, the others into d_pcm, from where one resampler launch
// per distinct rate writes them to d_mono -- and fingerprinted, under the uploads of the next group.
namespace {
// Uploads streams [begin, end) of a batch: stream i's plane c goes to d_raw + raw_off[i - begin] + c * plane_units[i - begin]
// on `up`; `issued` is told the stream's index in the batch once its last plane is on its way.
using FormatUpload = std::function<Status(size_t begin, size_t end, const std::vector<uint64_t> &raw_off,
                                          const std::vector<uint64_t> &plane_units, int16_t *d_raw, hipStream_t up,
                                          const StreamIssued &issued)>;

Status fingerprint_formats_in_batches(const std::vector<FormatWindow> &streams, bool any_mix, uint32_t step,
                                      std::vector<std::vector<uint32_t>> *items, uint32_t *d_items_out,
                                      const std::vector<uint64_t> *item_off_out, const FormatUpload &upload) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s;
  const size_t n = streams.size();
  for (const FormatWindow &w : streams)  // before any device is asked for
    if (!(s = lane_format_check(NeedleHipLaneFormat{w.channels, w.rate, w.format}, w.mix, "fingerprint")).ok()) return s;
  if (d_items_out && (!item_off_out || item_off_out->size() != n))
    return Status::Make(NeedleError_InvalidArgument, "fingerprint: one item offset per stream is required");
  if (step == 0) return Status::Make(NeedleError_InvalidArgument, "fingerprint: step must be >= 1");
  if (!(s = ensure_device()).ok()) return s;
  if (items) items->assign(n, {});
  bool count_values = false;
  const uint64_t kMaxBatchValues = batch_limit(&count_values);  // 2 GiB of raw samples, counted in s16 units
  uint64_t group_values = (32ull << 20) / sizeof(int16_t);
  if (const char *e = getenv("NEEDLE_HIP_LAUNCH_GROUP_BYTES")) group_values = (uint64_t)std::max(2ll, atoll(e)) / sizeof(int16_t);
  hipStream_t stream = library_stream(), up = upload_stream();
  struct DrainUploads {  // every exit waits for the copies already enqueued: they read the caller's buffers
    hipStream_t s;
    ~DrainUploads() { (void)hipStreamSynchronize(s); }
  } drain_uploads{up};
  OverlapEvents *ev = overlap_events();
  HostEntryWorkspace *ws = host_entry_workspace();
  DeviceBuffer<int16_t> &d_pcm = ws->d_pcm, &d_mono = ws->d_mono, &d_raw = ws->d_raw;
  DeviceBuffer<uint32_t> &d_items = ws->d_items;
  size_t begin = 0, descriptor_slot = 0;
  bool first_batch = true;
  while (begin < n) {
    struct Place {
      uint64_t raw, plane_units, staged, mono, out_samples;  // offsets in d_raw, d_pcm (resampled streams) and d_mono
    };
    std::vector<Place> place;
    std::vector<StreamSpan> spans;
    uint64_t raw = 0, raw_cost = 0, staged = 0, mono = 0, kept = 0;
    size_t end = begin;
    while (end < n) {
      const FormatWindow &w = streams[end];
      const size_t P = sample_format_planes(w.format, w.channels);
      const uint64_t plane_units = sample_plane_units(w.frames * (P == 1 ? (uint64_t)w.channels : 1), sample_format_width(w.format));
      const uint64_t cost = count_values ? w.frames * (uint64_t)w.channels : P * plane_units;
      if (end > begin && raw_cost + cost > kMaxBatchValues) break;
      const uint64_t out_samples = w.rate != kSampleRate ? resample_out_len(w.frames, w.rate) : w.frames;
      place.push_back(Place{raw, plane_units, staged, mono, out_samples});
      spans.push_back(StreamSpan{mono, out_samples, d_items_out ? (*item_off_out)[end] : kept});
      raw += P * plane_units;
      raw_cost += cost;
      if (w.rate != kSampleRate) staged += (w.frames + 7) & ~(uint64_t)7;
      mono += (out_samples + 7) & ~(uint64_t)7;
      kept += num_kept(out_samples, step);
      end++;
    }
    if (!(s = d_raw.reserve(std::max<uint64_t>(raw, 1))).ok()) return s;
    if (!(s = d_pcm.reserve(std::max<uint64_t>(staged, 1))).ok()) return s;
    if (!(s = d_mono.reserve(std::max<uint64_t>(mono, 1))).ok()) return s;
    if (!d_items_out && !(s = d_items.reserve(std::max<uint64_t>(kept, 1))).ok()) return s;
    uint32_t *const d_out = d_items_out ? d_items_out : d_items.ptr;
    // the copies must not overtake kernels that still read the arenas: those of the previous batch, or of an earlier call
    NEEDLE_HIP_TRY(hipEventRecord(first_batch ? ev->entry : ev->batch_done, stream));
    NEEDLE_HIP_TRY(hipStreamWaitEvent(up, first_batch ? ev->entry : ev->batch_done, 0));
    first_batch = false;
    size_t launched = 0;
    uint64_t pending_values = 0;
    auto launch_group = [&](size_t upto) -> Status {  // streams [launched, upto) of the batch have been enqueued on `up`
      if (upto <= launched) return Status::Ok();
      NEEDLE_HIP_TRY(hipEventRecord(ev->landed, up));
      NEEDLE_HIP_TRY(hipStreamWaitEvent(stream, ev->landed, 0));
      std::vector<IngestSpan> land;
      std::map<int, std::vector<ResampleSpan>> by_rate;
      for (size_t k = launched; k < upto; k++) {
        const FormatWindow &w = streams[begin + k];
        if (w.frames == 0) continue;
        IngestSpan in{};
        for (size_t c = 0; c < sample_format_planes(w.format, w.channels); c++) in.src[c] = d_raw.ptr + place[k].raw + c * place[k].plane_units;
        in.frames = w.frames;
        in.channels = w.channels;
        in.format = w.format;
        in.mix = w.mix;
        if (w.rate != kSampleRate) {
          in.dst = d_pcm.ptr + place[k].staged;
          by_rate[w.rate].push_back(ResampleSpan{place[k].staged, w.frames, place[k].mono});
        } else {
          in.dst = d_mono.ptr + place[k].mono;
        }
        land.push_back(in);
      }
      Status gs = land.empty() ? Status::Ok() : any_mix ? gpu_rematrix_device(land, false) : gpu_ingest_device(land, false);
      for (const auto &rs : by_rate)
        if (gs.ok()) gs = gpu_resample_device(d_pcm.ptr, rs.second, 1, rs.first, d_mono.ptr, false);
      const std::vector<StreamSpan> group(spans.begin() + launched, spans.begin() + upto);
      if (gs.ok()) gs = gpu_fingerprint_device(d_mono.ptr, group, 1, step, d_out, false, nullptr, nullptr, descriptor_slot++);
      launched = upto;
      pending_values = 0;
      return gs;
    };
    std::vector<uint64_t> raw_off, plane_units;
    for (const Place &p : place) {
      raw_off.push_back(p.raw);
      plane_units.push_back(p.plane_units);
    }
    const StreamIssued issued = [&](size_t i) -> Status {  // i: index inside the batch
      const FormatWindow &w = streams[begin + i];
      pending_values += w.frames * (uint64_t)w.channels;
      return pending_values >= group_values ? launch_group(i + 1) : Status::Ok();
    };
    if (!(s = upload(begin, end, raw_off, plane_units, d_raw.ptr, up, issued)).ok()) return s;
    if (!(s = launch_group(end - begin)).ok()) return s;
    if (items) {
      std::vector<uint32_t> host(std::max<uint64_t>(kept, 1));
      NEEDLE_HIP_TRY(hipMemcpyAsync(host.data(), d_items.ptr, kept * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
      for (size_t i = begin; i < end; i++) {
        const size_t k = num_kept(place[i - begin].out_samples, step);
        (*items)[i].assign(host.begin() + spans[i - begin].item_off, host.begin() + spans[i - begin].item_off + k);
      }
    }
    begin = end;
  }
  NEEDLE_HIP_TRY(hipStreamSynchronize(up));
  return Status::Ok();
}
}  // namespace

Status gpu_fingerprint_formats(const std::vector<FormatWindow> &streams, bool any_mix, uint32_t step,
                               std::vector<std::vector<uint32_t>> *items, uint32_t *d_items_out,
                               const std::vector<uint64_t> *item_off_out) {
  const FormatUpload from_pointers = [&](size_t begin, size_t end, const std::vector<uint64_t> &raw_off,
                                         const std::vector<uint64_t> &plane_units, int16_t *d_raw, hipStream_t up,
                                         const StreamIssued &issued) -> Status {
    std::vector<const void *> src;
    std::vector<size_t> bytes, stream_of_plane;
    std::vector<uint64_t> off;
    std::vector<char> last_plane;
    for (size_t i = begin; i < end; i++) {
      const FormatWindow &w = streams[i];
      const size_t P = sample_format_planes(w.format, w.channels);
      for (size_t c = 0; c < P; c++) {
        src.push_back(w.src[c]);
        bytes.push_back(w.frames * (P == 1 ? (uint64_t)w.channels : 1) * sample_format_width(w.format));
        off.push_back(raw_off[i - begin] + c * plane_units[i - begin]);
        stream_of_plane.push_back(i - begin);
        last_plane.push_back(c + 1 == P);
      }
    }
    const StreamIssued plane_issued = [&](size_t k) -> Status { return last_plane[k] ? issued(stream_of_plane[k]) : Status::Ok(); };
    return gpu_upload_raw(src, bytes, off, d_raw, up, plane_issued);
  };
  return fingerprint_formats_in_batches(streams, any_mix, step, items, d_items_out, item_off_out, from_pointers);
}

Status gpu_fingerprint_formats_streamed(const std::vector<FormatWindow> &streams, bool any_mix, const PcmReader &read, unsigned readers,
                                        uint32_t step, std::vector<std::vector<uint32_t>> *items) {
  for (const FormatWindow &w : streams)
    if (w.format != NEEDLE_HIP_SAMPLE_S16) return Status::Make(NeedleError_InvalidArgument, "fingerprint: a reader produces interleaved s16");
  const FormatUpload from_reader = [&](size_t begin, size_t end, const std::vector<uint64_t> &raw_off, const std::vector<uint64_t> &,
                                       int16_t *d_raw, hipStream_t up, const StreamIssued &issued) -> Status {
    std::vector<size_t> num_values;
    for (size_t i = begin; i < end; i++) num_values.push_back(streams[i].frames * (size_t)streams[i].channels);
    const PcmReader shifted = [&](size_t stream, uint64_t first, uint64_t count, int16_t *dst) { return read(begin + stream, first, count, dst); };
    return gpu_upload_pcm_streamed(num_values, raw_off, shifted, readers, d_raw, up, issued);
  };
  return fingerprint_formats_in_batches(streams, any_mix, step, items, nullptr, nullptr, from_reader);
}

}  // namespace needle
