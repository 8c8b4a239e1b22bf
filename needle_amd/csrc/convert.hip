// GPU sample-format conversion: PCM as a decoder hands it over (u8 / s16 / s32 / f32 / f64, interleaved or one plane
// per channel) -> the s16 the rest of the path reads.  The arithmetic is the WAV reader's (hostutil.cpp wav_convert),
// this front end's own specification, per sample:
//   u8 : (x - 128) << 8            s16: x            s32: x >> 16 (arithmetic: the two most significant bytes)
//   f32: y = rintf(x * 32768.0f) (ties to even), NaN -> 0, otherwise clipped to [-32768, 32767]
//   f64: the same in f64 (never through f32: (0.5 + 2^-30) / 32768 converts to 1, and to 0 if narrowed first)
// Output is interleaved C-channel s16 (Mix = false), or mono s16 with downmix.hip's down-mix fused in (Mix = true):
// (sum of the frame's C converted values) / C, C integer division.  A trailing partial frame is dropped by the caller.
//
// A streaming, memory-bound kernel in the mould of downmix.hip: each lane takes 8 consecutive frames (16 of u8, so
// that a plane's share is a whole 16-byte load), reads them with 16-byte loads -- FPL * C * sizeof(T) contiguous bytes
// of an interleaved stream, FPL * sizeof(T) of each plane -- and writes 16-byte stores.  Format and C are template
// parameters (the division is by a constant).  One launch covers every stream of a group: the streams are cut into
// virtual blocks of 256 lanes' frames, a workgroup walks virtual blocks with a grid stride and finds the stream of each
// by a binary search over the table's block bases.  Sources that are not 16-byte aligned (a caller's device pointer is
// only aligned to its sample) and the last few frames of a stream take a scalar path.  Output goes to a buffer of
// its own.  Interleaved input that is not mixed is converted value by value, whatever C is (the C = 1 kernel).
#include "hipctx.h"
#include "ingest_block.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>

namespace needle {

namespace {

struct CvStream {
  const void *src[NEEDLE_HIP_MAX_CHANNELS];  // planar: plane c; interleaved: src[0]
  int16_t *dst;
  uint64_t frames;
  uint64_t block_base;  // first virtual block of this stream
};

}  // namespace

// (outside the anonymous namespace: one readable name in kernel traces, convert_kernel<T, Planar, C, Mix>)
template <typename T, bool Planar, int C, bool Mix>
__global__ __launch_bounds__(kCvThreads) void convert_kernel(const CvStream *__restrict__ streams, int n, uint64_t blocks) {
  constexpr int FPL = frames_per_lane<T>();
  constexpr int OUT = Mix ? 1 : C;  // s16 values written per frame
  constexpr uint64_t kFramesPerBlock = (uint64_t)kCvThreads * FPL;
  for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
    int lo = 0, hi = n - 1;  // last stream whose block_base <= b (zero-frame streams are not in the table)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (streams[mid].block_base <= b) lo = mid;
      else hi = mid - 1;
    }
    const CvStream &st = streams[lo];
    const uint64_t frames = st.frames;
    const uint64_t f0 = (b - st.block_base) * kFramesPerBlock + (uint64_t)threadIdx.x * FPL;
    if (f0 >= frames) continue;
    int16_t *y = st.dst + f0 * OUT;
    const T *x[Planar ? C : 1];  // the lane's first sample of every plane / of the interleaved stream
    uintptr_t align = 0;
#pragma unroll
    for (int c = 0; c < (Planar ? C : 1); c++) {
      x[c] = static_cast<const T *>(st.src[c]) + f0 * (Planar ? 1 : C);
      align |= reinterpret_cast<uintptr_t>(x[c]);
    }
    if (f0 + FPL <= frames && (align & 15) == 0) {
      T v[FPL * C];  // frame-major: v[f * C + c]
      if (Planar) {
        constexpr int NV = FPL * (int)sizeof(T) / 16;
#pragma unroll
        for (int c = 0; c < C; c++) {
          uint4 raw[NV];
#pragma unroll
          for (int k = 0; k < NV; k++) raw[k] = reinterpret_cast<const uint4 *>(x[c])[k];
          T p[FPL];
          __builtin_memcpy(p, raw, sizeof(raw));
#pragma unroll
          for (int f = 0; f < FPL; f++) v[f * C + c] = p[f];
        }
      } else {
        constexpr int NV = FPL * C * (int)sizeof(T) / 16;
        uint4 raw[NV];
#pragma unroll
        for (int k = 0; k < NV; k++) raw[k] = reinterpret_cast<const uint4 *>(x[0])[k];
        __builtin_memcpy(v, raw, sizeof(raw));
      }
      uint32_t w[FPL * OUT / 2];  // two s16 per word
#pragma unroll
      for (int i = 0; i < FPL * OUT / 2; i++) {
        int s[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
          if (Mix) {
            int sum = 0;
#pragma unroll
            for (int c = 0; c < C; c++) sum += to_s16<T>(v[(2 * i + h) * C + c]);
            s[h] = sum / C;
          } else {
            s[h] = to_s16<T>(v[2 * i + h]);
          }
        }
        w[i] = (uint32_t)(uint16_t)(int16_t)s[0] | ((uint32_t)(uint16_t)(int16_t)s[1] << 16);
      }
      if ((reinterpret_cast<uintptr_t>(y) & 15) == 0) {
#pragma unroll
        for (int k = 0; k < FPL * OUT / 8; k++)
          reinterpret_cast<uint4 *>(y)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
      } else {
#pragma unroll
        for (int i = 0; i < FPL * OUT / 2; i++) {
          y[2 * i] = (int16_t)(w[i] & 0xFFFF);
          y[2 * i + 1] = (int16_t)(w[i] >> 16);
        }
      }
    } else {
      const int nf = frames - f0 < (uint64_t)FPL ? (int)(frames - f0) : FPL;
      for (int f = 0; f < nf; f++) {
        int sum = 0;
#pragma unroll
        for (int c = 0; c < C; c++) {
          const int s = to_s16<T>(Planar ? x[c][f] : x[0][(size_t)f * C + c]);
          if (Mix) sum += s;
          else y[(size_t)f * C + c] = (int16_t)s;
        }
        if (Mix) y[f] = (int16_t)(sum / C);
      }
    }
  }
}

// ---- the ingest of a feeder whose lanes have formats of their own: IngestStream and ingest_block, ingest_block.h ---

// (a span's virtual blocks are of its own sample type's size: the table's block bases are counted on the host)
__global__ __launch_bounds__(kCvThreads) void feeder_ingest_kernel(const IngestStream *__restrict__ streams, int n, uint64_t blocks) {
  for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
    int lo = 0, hi = n - 1;  // last span whose block_base <= b (zero-frame spans are not in the table)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (streams[mid].block_base <= b) lo = mid;
      else hi = mid - 1;
    }
    const IngestStream *st = streams + lo;
    const uint64_t block = b - st->block_base;
    switch (st->type) {
      case NEEDLE_HIP_SAMPLE_U8: ingest_block<uint8_t>(st, block); break;
      case NEEDLE_HIP_SAMPLE_S16: ingest_block<int16_t>(st, block); break;
      case NEEDLE_HIP_SAMPLE_S32: ingest_block<int32_t>(st, block); break;
      case NEEDLE_HIP_SAMPLE_F32: ingest_block<float>(st, block); break;
      default: ingest_block<double>(st, block); break;
    }
  }
}

namespace {

using CvKernel = void (*)(const CvStream *, int, uint64_t);

template <typename T, bool Planar, bool Mix>
CvKernel pick_channels(int channels) {
  switch (channels) {
    case 3: return convert_kernel<T, Planar, 3, Mix>;
    case 4: return convert_kernel<T, Planar, 4, Mix>;
    case 5: return convert_kernel<T, Planar, 5, Mix>;
    case 6: return convert_kernel<T, Planar, 6, Mix>;
    case 7: return convert_kernel<T, Planar, 7, Mix>;
    case 8: return convert_kernel<T, Planar, 8, Mix>;
    default: break;
  }
  if constexpr (!Mix) {  // (1 and 2 channels are never mixed here: the STFT and the resampler read stereo themselves)
    if (channels == 2) return convert_kernel<T, Planar, 2, false>;
    if (channels == 1) return convert_kernel<T, false, 1, false>;
  }
  return nullptr;
}

template <typename T>
CvKernel pick_layout(bool planar, int channels, bool mix) {
  if (mix) return planar ? pick_channels<T, true, true>(channels) : pick_channels<T, false, true>(channels);
  // interleaved in, interleaved out: value by value
  return planar ? pick_channels<T, true, false>(channels) : convert_kernel<T, false, 1, false>;
}

CvKernel pick_kernel(int format, int channels, bool mix) {
  const bool planar = sample_format_planar(format);
  switch (format % 5) {
    case NEEDLE_HIP_SAMPLE_U8: return pick_layout<uint8_t>(planar, channels, mix);
    case NEEDLE_HIP_SAMPLE_S16: return pick_layout<int16_t>(planar, channels, mix);
    case NEEDLE_HIP_SAMPLE_S32: return pick_layout<int32_t>(planar, channels, mix);
    case NEEDLE_HIP_SAMPLE_F32: return pick_layout<float>(planar, channels, mix);
    default: return pick_layout<double>(planar, channels, mix);
  }
}

}  // namespace

Status gpu_convert_device(const std::vector<ConvertSpan> &spans, int channels, int format, bool mix, bool sync) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  if (channels < 1 || channels > NEEDLE_HIP_MAX_CHANNELS)
    return Status::Make(NeedleError_InvalidArgument, "convert: channels must be 1 to " + std::to_string(NEEDLE_HIP_MAX_CHANNELS));
  if (!sample_format_valid(format)) return Status::Make(NeedleError_InvalidArgument, "convert: unknown sample format");
  if (mix && channels < 3) return Status::Make(NeedleError_InvalidArgument, "convert: the fused down-mix is for 3 to 8 channels");
  Status s = ensure_device();
  if (!s.ok()) return s;
  int dev = 0;
  NEEDLE_HIP_TRY(hipGetDevice(&dev));
  const bool planar = sample_format_planar(format) && channels > 1;
  const bool by_value = !planar && !mix;  // the C = 1 kernel over frames * C values
  const uint64_t lane_frames = sample_format_width(format) == 1 ? 16 : 8;
  const uint64_t block_frames = (uint64_t)kCvThreads * lane_frames;
  std::vector<CvStream> meta;
  uint64_t blocks = 0;
  for (const ConvertSpan &sp : spans) {
    if (sp.frames == 0) continue;
    CvStream st{};
    for (int c = 0; c < (planar ? channels : 1); c++) {
      if (!sp.src[c]) return Status::Make(NeedleError_NullArgument, "convert: null stream pointer");
      st.src[c] = sp.src[c];
    }
    if (!sp.dst) return Status::Make(NeedleError_NullArgument, "convert: null stream pointer");
    st.dst = sp.dst;
    st.frames = by_value ? sp.frames * (uint64_t)channels : sp.frames;
    st.block_base = blocks;
    meta.push_back(st);
    blocks += (st.frames + block_frames - 1) / block_frames;
  }
  if (meta.size() > 0x7FFFFFFFull) return Status::Make(NeedleError_InvalidArgument, "convert: too many streams for one launch");
  hipStream_t stream = library_stream();
  if (!meta.empty()) {
    const CvKernel kernel = pick_kernel(format, channels, mix);
    if (!kernel) return Status::Make(NeedleError_Unknown, "convert: no kernel for this format and channel count");
    // descriptor table: per device, pinned staging, in stream order behind the previous launch (as the down-mix's)
    static std::map<int, std::pair<DeviceBuffer<CvStream> *, PinnedStage *>> ws;
    auto &w = ws[dev];
    if (!w.first) {
      w.first = new DeviceBuffer<CvStream>();
      w.second = new PinnedStage();
    }
    if (!(s = w.first->reserve(meta.size())).ok()) return s;
    if (!(s = w.second->acquire(meta.size() * sizeof(CvStream))).ok()) return s;
    std::memcpy(w.second->ptr, meta.data(), meta.size() * sizeof(CvStream));
    NEEDLE_HIP_TRY(hipMemcpyAsync(w.first->ptr, w.second->ptr, meta.size() * sizeof(CvStream), hipMemcpyHostToDevice, stream));
    w.second->mark(stream);
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(blocks, (uint64_t)std::max(cus, 1) * 8);  // the rest by grid stride
    KernelTimer timer("convert");
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kCvThreads), 0, stream, w.first->ptr, (int)meta.size(), blocks);
    NEEDLE_HIP_TRY(hipGetLastError());
  }
  if (sync) NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  return Status::Ok();
}

Status gpu_upload_raw(const std::vector<const void *> &src, const std::vector<size_t> &bytes, const std::vector<uint64_t> &dev_off,
                      int16_t *d_raw, hipStream_t stream, const StreamIssued &issued) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = ensure_device();
  if (!s.ok()) return s;
  if (!stream) stream = library_stream();
  std::vector<const int16_t *> pcm(src.size());
  std::vector<size_t> values(src.size());
  for (size_t i = 0; i < src.size(); i++) {
    pcm[i] = static_cast<const int16_t *>(src[i]);
    values[i] = bytes[i] / 2;
    if (bytes[i] & 1)  // (u8 only) the odd last byte goes first: every copy of a stream is enqueued before `issued` hears of it
      NEEDLE_HIP_TRY(hipMemcpyAsync(reinterpret_cast<uint8_t *>(d_raw + dev_off[i]) + bytes[i] - 1,
                                    static_cast<const uint8_t *>(src[i]) + bytes[i] - 1, 1, hipMemcpyHostToDevice, stream));
  }
  return gpu_upload_pcm(pcm, values, dev_off, d_raw, stream, issued);
}

Status gpu_convert_host(const std::vector<const void *> &pcm, const std::vector<size_t> &num_values, int channels, int format,
                        const std::vector<int16_t *> &out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  if (channels < 1 || channels > NEEDLE_HIP_MAX_CHANNELS)
    return Status::Make(NeedleError_InvalidArgument, "convert: channels must be 1 to " + std::to_string(NEEDLE_HIP_MAX_CHANNELS));
  if (!sample_format_valid(format)) return Status::Make(NeedleError_InvalidArgument, "convert: unknown sample format");
  const uint64_t C = (uint64_t)channels, W = sample_format_width(format);
  const size_t P = sample_format_planar(format) ? (size_t)channels : 1;  // pointers per stream
  if (pcm.size() != num_values.size() * P || out.size() != num_values.size())
    return Status::Make(NeedleError_InvalidArgument, "convert: one length and one output per stream, one pointer per plane are required");
  Status s = ensure_device();
  if (!s.ok()) return s;
  // Batches of at most NEEDLE_HIP_MAX_BATCH_VALUES input values (2 GiB of raw samples by default); a stream longer than
  // that is cut into pieces of whole 16-frame groups (frames are independent of each other).
  uint64_t max_values = (2ull << 30) / W;
  if (const char *e = getenv("NEEDLE_HIP_MAX_BATCH_VALUES")) max_values = (uint64_t)std::max(1ll, atoll(e));  // tests
  const uint64_t piece_frames = std::max<uint64_t>(16, max_values / C / 16 * 16);
  auto plane_units = [&](uint64_t frames) {  // s16 units one staged plane (or interleaved piece) takes, 16-byte aligned
    return ((frames * (P == 1 ? C : 1) * W + 15) & ~(uint64_t)15) / 2;
  };
  struct Piece {
    size_t stream;
    uint64_t first, frames, in_off, out_off;
  };
  std::vector<Piece> pieces;
  for (size_t i = 0; i < num_values.size(); i++) {
    const uint64_t frames = num_values[i] / C;
    for (uint64_t f = 0; f < frames; f += piece_frames) pieces.push_back(Piece{i, f, std::min(piece_frames, frames - f), 0, 0});
  }
  hipStream_t stream = library_stream();
  DeviceBuffer<int16_t> d_in, d_out;
  size_t begin = 0;
  while (begin < pieces.size()) {
    uint64_t values = 0, in_total = 0, out_total = 0;
    size_t end = begin;
    while (end < pieces.size() && (end == begin || values + pieces[end].frames * C <= max_values)) {
      pieces[end].in_off = in_total;
      pieces[end].out_off = out_total;
      values += pieces[end].frames * C;
      in_total += plane_units(pieces[end].frames) * P;
      out_total += (pieces[end].frames * C + 7) & ~(uint64_t)7;
      end++;
    }
    if (!(s = d_in.reserve(in_total)).ok() || !(s = d_out.reserve(out_total)).ok()) return s;
    std::vector<const void *> src;
    std::vector<size_t> len;
    std::vector<uint64_t> off;
    std::vector<ConvertSpan> spans;
    for (size_t k = begin; k < end; k++) {
      const Piece &p = pieces[k];
      if (!out[p.stream]) return Status::Make(NeedleError_NullArgument, "convert: null stream pointer");
      ConvertSpan sp{};
      for (size_t c = 0; c < P; c++) {
        const void *plane = pcm[p.stream * P + c];
        if (!plane) return Status::Make(NeedleError_NullArgument, "convert: null stream pointer");
        src.push_back(static_cast<const uint8_t *>(plane) + p.first * (P == 1 ? C : 1) * W);
        len.push_back(p.frames * (P == 1 ? C : 1) * W);
        off.push_back(p.in_off + c * plane_units(p.frames));
        sp.src[c] = d_in.ptr + off.back();
      }
      sp.dst = d_out.ptr + p.out_off;
      sp.frames = p.frames;
      spans.push_back(sp);
    }
    s = gpu_upload_raw(src, len, off, d_in.ptr, stream);
    if (s.ok()) s = gpu_convert_device(spans, channels, format, false, false);
    // also on the error path: copies already enqueued read the caller's buffers asynchronously
    const bool drained = hipStreamSynchronize(stream) == hipSuccess;
    if (!s.ok()) return s;
    if (!drained) return Status::Make(NeedleError_Unknown, "convert: upload or kernel failed");
    for (size_t k = begin; k < end; k++) {
      const Piece &p = pieces[k];
      NEEDLE_HIP_TRY(hipMemcpy(out[p.stream] + p.first * C, d_out.ptr + p.out_off, p.frames * C * sizeof(int16_t), hipMemcpyDeviceToHost));
    }
    begin = end;
  }
  return Status::Ok();
}

Status gpu_ingest_device(const std::vector<IngestSpan> &spans, bool sync) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = ensure_device();
  if (!s.ok()) return s;
  int dev = 0;
  NEEDLE_HIP_TRY(hipGetDevice(&dev));
  std::vector<IngestStream> meta;
  uint64_t blocks = 0;
  for (const IngestSpan &sp : spans) {
    IngestStream st{};
    if (!(s = ingest_stream_of(sp, &blocks, &st)).ok()) return s;
    if (st.frames) meta.push_back(st);
  }
  if (meta.size() > 0x7FFFFFFFull) return Status::Make(NeedleError_InvalidArgument, "ingest: too many spans for one launch");
  hipStream_t stream = library_stream();
  if (!meta.empty()) {
    // descriptor table: per device, pinned staging, in stream order behind the previous launch (as the conversion's)
    static std::map<int, std::pair<DeviceBuffer<IngestStream> *, PinnedStage *>> ws;
    auto &w = ws[dev];
    if (!w.first) {
      w.first = new DeviceBuffer<IngestStream>();
      w.second = new PinnedStage();
    }
    if (!(s = w.first->reserve(meta.size())).ok()) return s;
    if (!(s = w.second->acquire(meta.size() * sizeof(IngestStream))).ok()) return s;
    std::memcpy(w.second->ptr, meta.data(), meta.size() * sizeof(IngestStream));
    NEEDLE_HIP_TRY(hipMemcpyAsync(w.first->ptr, w.second->ptr, meta.size() * sizeof(IngestStream), hipMemcpyHostToDevice, stream));
    w.second->mark(stream);
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(blocks, (uint64_t)std::max(cus, 1) * 8);  // the rest by grid stride
    KernelTimer timer("ingest");
    hipLaunchKernelGGL(feeder_ingest_kernel, dim3(grid), dim3(kCvThreads), 0, stream, w.first->ptr, (int)meta.size(), blocks);
    NEEDLE_HIP_TRY(hipGetLastError());
  }
  if (sync) NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  return Status::Ok();
}

Status gpu_convert_mono_host(const std::vector<const void *> &pcm, const std::vector<size_t> &num_values,
                             const std::vector<int> &channels, const std::vector<int> &formats, const std::vector<int16_t *> &out,
                             const NeedleHipChannelMix *mixes) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  const size_t n = num_values.size();
  if (channels.size() != n || formats.size() != n || out.size() != n)
    return Status::Make(NeedleError_InvalidArgument, "ingest: one length, one format and one output per stream are required");
  std::vector<size_t> first_plane(n + 1, 0);  // of stream i in pcm
  for (size_t i = 0; i < n; i++) {
    if (channels[i] < 1 || channels[i] > NEEDLE_HIP_MAX_CHANNELS)
      return Status::Make(NeedleError_InvalidArgument, "ingest: channels must be 1 to " + std::to_string(NEEDLE_HIP_MAX_CHANNELS));
    if (!sample_format_valid(formats[i])) return Status::Make(NeedleError_InvalidArgument, "ingest: unknown sample format");
    if (mixes && mixes[i].channels) {
      Status ms = channel_mix_check(mixes[i], channels[i]);
      if (!ms.ok()) return ms;
    }
    first_plane[i + 1] = first_plane[i] + sample_format_planes(formats[i], channels[i]);
  }
  if (pcm.size() != first_plane[n]) return Status::Make(NeedleError_InvalidArgument, "ingest: one pointer per stream and plane is required");
  // Batches of at most NEEDLE_HIP_MAX_BATCH_VALUES input values (2^30 by default); a stream longer than that is cut into
  // pieces of whole 16-frame groups (frames are independent of each other).
  uint64_t max_values = 1ull << 30;
  if (const char *e = getenv("NEEDLE_HIP_MAX_BATCH_VALUES")) max_values = (uint64_t)std::max(1ll, atoll(e));  // tests
  struct Piece {
    size_t stream;
    uint64_t first, frames, in_off, out_off;
  };
  std::vector<Piece> pieces;
  for (size_t i = 0; i < n; i++) {
    const uint64_t C = (uint64_t)channels[i], frames = num_values[i] / C;
    const uint64_t piece_frames = std::max<uint64_t>(16, max_values / C / 16 * 16);
    for (uint64_t f = 0; f < frames; f += piece_frames) pieces.push_back(Piece{i, f, std::min(piece_frames, frames - f), 0, 0});
  }
  if (pieces.empty()) return Status::Ok();  // no whole frame anywhere: nothing is read or written
  Status s = ensure_device();
  if (!s.ok()) return s;
  // A staged plane keeps its pointer's offset from 16-byte alignment (a piece starts a multiple of 16 bytes behind its
  // plane), so the kernel takes the path the caller's own pointers ask for.
  auto plane_units = [&](const Piece &p) {
    const uint64_t C = (uint64_t)channels[p.stream], P = first_plane[p.stream + 1] - first_plane[p.stream];
    return sample_plane_units(p.frames * (P == 1 ? C : 1), sample_format_width(formats[p.stream])) + 8;
  };
  hipStream_t stream = library_stream();
  DeviceBuffer<int16_t> d_in, d_out;
  size_t begin = 0;
  while (begin < pieces.size()) {
    uint64_t values = 0, in_total = 0, out_total = 0;
    size_t end = begin;
    while (end < pieces.size() && (end == begin || values + pieces[end].frames * (uint64_t)channels[pieces[end].stream] <= max_values)) {
      Piece &p = pieces[end];
      p.in_off = in_total;
      p.out_off = out_total;
      values += p.frames * (uint64_t)channels[p.stream];
      in_total += plane_units(p) * (first_plane[p.stream + 1] - first_plane[p.stream]);
      out_total += (p.frames + 7) & ~(uint64_t)7;
      end++;
    }
    if (!(s = d_in.reserve(in_total)).ok() || !(s = d_out.reserve(out_total)).ok()) return s;
    std::vector<IngestSpan> spans;
    s = Status::Ok();
    for (size_t k = begin; k < end && s.ok(); k++) {
      const Piece &p = pieces[k];
      const uint64_t C = (uint64_t)channels[p.stream], W = sample_format_width(formats[p.stream]);
      const size_t P = first_plane[p.stream + 1] - first_plane[p.stream];
      IngestSpan sp{};
      for (size_t c = 0; c < P && s.ok(); c++) {
        const void *plane = pcm[first_plane[p.stream] + c];
        if (!plane || !out[p.stream]) {
          s = Status::Make(NeedleError_NullArgument, "ingest: null stream pointer");
          break;
        }
        const uint8_t *from = static_cast<const uint8_t *>(plane) + p.first * (P == 1 ? C : 1) * W;
        uint8_t *at = reinterpret_cast<uint8_t *>(d_in.ptr + p.in_off + c * plane_units(p)) + (reinterpret_cast<uintptr_t>(from) & 15);
        const hipError_t e = hipMemcpyAsync(at, from, p.frames * (P == 1 ? C : 1) * W, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) s = Status::Make(NeedleError_Unknown, std::string("HIP error: ") + hipGetErrorString(e));
        sp.src[c] = at;
      }
      sp.dst = d_out.ptr + p.out_off;
      sp.frames = p.frames;
      sp.channels = channels[p.stream];
      sp.format = formats[p.stream];
      if (mixes && mixes[p.stream].channels) sp.mix = &mixes[p.stream];
      spans.push_back(sp);
    }
    if (s.ok()) s = mixes ? gpu_rematrix_device(spans, false) : gpu_ingest_device(spans, false);
    // also on the error path: copies already enqueued read the caller's buffers asynchronously
    const bool drained = hipStreamSynchronize(stream) == hipSuccess;
    if (!s.ok()) return s;
    if (!drained) return Status::Make(NeedleError_Unknown, "ingest: upload or kernel failed");
    for (size_t k = begin; k < end; k++) {
      const Piece &p = pieces[k];
      NEEDLE_HIP_TRY(hipMemcpy(out[p.stream] + p.first, d_out.ptr + p.out_off, p.frames * sizeof(int16_t), hipMemcpyDeviceToHost));
    }
    begin = end;
  }
  return Status::Ok();
}

}  // namespace needle
