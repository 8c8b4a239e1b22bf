// GPU down-mix: interleaved C-channel s16 -> mono s16, the first step of the path for 3-8 channel (surround) input.
// The arithmetic is the front end's own specification (oracle/ora_resample.h, chromaprint's AudioProcessor):
//   mono[n] = (int)(sum over c of x[n * C + c]) / C      (C integer division: truncation toward zero)
// and a trailing partial frame (num_values % C) is dropped.  The sum of at most 8 s16 values fits an int, and the
// quotient of such a sum by C lies in the s16 range, so the result is exact.
//
// A streaming, memory-bound kernel: each lane takes 8 consecutive frames, i.e. C contiguous 16-byte loads and one
// 16-byte store, so the lanes of a wave read one contiguous stretch of 1 KiB x C.  C is a template parameter, so
// the division is by a constant (a multiply-high and shifts).  One launch covers every stream of a group: the
// streams are cut into virtual blocks of 2048 frames, a workgroup walks virtual blocks with a grid stride and finds
// the stream of each by a binary search over the table's block bases (uniform across the workgroup).  Sources or
// destinations that are not 16-byte aligned (a caller's device pointer is only 2-byte aligned) and the last few
// frames of a stream take a scalar path.  Output always goes to a separate buffer: compacting in place would race
// across workgroups.
#include "hipctx.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>

namespace needle {

namespace {

constexpr int kDmThreads = 256;
constexpr int kDmFramesPerLane = 8;
constexpr uint64_t kDmFramesPerBlock = (uint64_t)kDmThreads * kDmFramesPerLane;

struct DmStream {
  const int16_t *src;   // interleaved C-channel frames
  int16_t *dst;         // mono
  uint64_t frames;
  uint64_t block_base;  // first virtual block of this stream
};

template <int C>
__device__ __forceinline__ int16_t mix_frame(const int16_t *x) {
  int sum = 0;
#pragma unroll
  for (int c = 0; c < C; c++) sum += x[c];
  return (int16_t)(sum / C);
}

}  // namespace

// (outside the anonymous namespace: the kernel keeps one readable name in kernel traces, downmix_kernel<C>)
template <int C>
__global__ __launch_bounds__(kDmThreads) void downmix_kernel(const DmStream *__restrict__ streams, int n, uint64_t blocks) {
  for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
    int lo = 0, hi = n - 1;  // last stream whose block_base <= b (zero-frame streams are not in the table)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (streams[mid].block_base <= b) lo = mid;
      else hi = mid - 1;
    }
    const DmStream st = streams[lo];
    const uint64_t f0 = (b - st.block_base) * kDmFramesPerBlock + (uint64_t)threadIdx.x * kDmFramesPerLane;
    if (f0 >= st.frames) continue;
    const int16_t *x = st.src + f0 * C;
    int16_t *y = st.dst + f0;
    if (f0 + kDmFramesPerLane <= st.frames && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
      uint32_t w[4 * C];  // the lane's 8 frames: 8 C values, two per word
#pragma unroll
      for (int k = 0; k < C; k++) {
        const uint4 v = reinterpret_cast<const uint4 *>(x)[k];
        w[4 * k] = v.x;
        w[4 * k + 1] = v.y;
        w[4 * k + 2] = v.z;
        w[4 * k + 3] = v.w;
      }
      uint32_t m[4];
#pragma unroll
      for (int p = 0; p < 4; p++) {
        int s0 = 0, s1 = 0;
#pragma unroll
        for (int c = 0; c < C; c++) {
          const int i0 = (2 * p) * C + c, i1 = (2 * p + 1) * C + c;
          s0 += (int)(int16_t)(w[i0 >> 1] >> ((i0 & 1) * 16));
          s1 += (int)(int16_t)(w[i1 >> 1] >> ((i1 & 1) * 16));
        }
        m[p] = (uint32_t)(uint16_t)(int16_t)(s0 / C) | ((uint32_t)(uint16_t)(int16_t)(s1 / C) << 16);
      }
      if ((reinterpret_cast<uintptr_t>(y) & 15) == 0) {
        *reinterpret_cast<uint4 *>(y) = make_uint4(m[0], m[1], m[2], m[3]);
      } else {
#pragma unroll
        for (int p = 0; p < 4; p++) {
          y[2 * p] = (int16_t)(m[p] & 0xFFFF);
          y[2 * p + 1] = (int16_t)(m[p] >> 16);
        }
      }
    } else {
      const int nf = st.frames - f0 < (uint64_t)kDmFramesPerLane ? (int)(st.frames - f0) : kDmFramesPerLane;
      for (int f = 0; f < nf; f++) y[f] = mix_frame<C>(x + (size_t)f * C);
    }
  }
}

Status gpu_downmix_device(const std::vector<DownmixSpan> &spans, int channels, bool sync) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  if (channels < 1 || channels > NEEDLE_HIP_MAX_CHANNELS)
    return Status::Make(NeedleError_InvalidArgument, "downmix: channels must be 1 to " + std::to_string(NEEDLE_HIP_MAX_CHANNELS));
  Status s = ensure_device();
  if (!s.ok()) return s;
  int dev = 0;
  NEEDLE_HIP_TRY(hipGetDevice(&dev));
  std::vector<DmStream> meta;
  uint64_t blocks = 0;
  for (const DownmixSpan &sp : spans) {
    if (sp.frames == 0) continue;
    if (!sp.src || !sp.dst) return Status::Make(NeedleError_NullArgument, "downmix: null stream pointer");
    meta.push_back(DmStream{sp.src, sp.dst, sp.frames, blocks});
    blocks += (sp.frames + kDmFramesPerBlock - 1) / kDmFramesPerBlock;
  }
  if (meta.size() > 0x7FFFFFFFull) return Status::Make(NeedleError_InvalidArgument, "downmix: too many streams for one launch");
  hipStream_t stream = library_stream();
  if (!meta.empty()) {
    // descriptor table: per device, pinned staging, in stream order behind the previous launch (as the resampler's)
    static std::map<int, std::pair<DeviceBuffer<DmStream> *, PinnedStage *>> ws;
    auto &w = ws[dev];
    if (!w.first) {
      w.first = new DeviceBuffer<DmStream>();
      w.second = new PinnedStage();
    }
    if (!(s = w.first->reserve(meta.size())).ok()) return s;
    if (!(s = w.second->acquire(meta.size() * sizeof(DmStream))).ok()) return s;
    std::memcpy(w.second->ptr, meta.data(), meta.size() * sizeof(DmStream));
    NEEDLE_HIP_TRY(hipMemcpyAsync(w.first->ptr, w.second->ptr, meta.size() * sizeof(DmStream), hipMemcpyHostToDevice, stream));
    w.second->mark(stream);
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    // a memory-bound stream: 8 workgroups per CU (48 KiB of loads in flight per CU at C = 6), the rest by grid stride
    const uint32_t grid = (uint32_t)std::min<uint64_t>(blocks, (uint64_t)std::max(cus, 1) * 8);
    KernelTimer timer("downmix");
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(kDmThreads), 0, stream, w.first->ptr, (int)meta.size(), blocks);
    };
    switch (channels) {
      case 1: launch(downmix_kernel<1>); break;
      case 2: launch(downmix_kernel<2>); break;
      case 3: launch(downmix_kernel<3>); break;
      case 4: launch(downmix_kernel<4>); break;
      case 5: launch(downmix_kernel<5>); break;
      case 6: launch(downmix_kernel<6>); break;
      case 7: launch(downmix_kernel<7>); break;
      default: launch(downmix_kernel<8>); break;
    }
    NEEDLE_HIP_TRY(hipGetLastError());
  }
  if (sync) NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  return Status::Ok();
}

Status gpu_downmix_host(const std::vector<const int16_t *> &pcm, const std::vector<size_t> &num_values, int channels,
                        const std::vector<int16_t *> &out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  if (channels < 1 || channels > NEEDLE_HIP_MAX_CHANNELS)
    return Status::Make(NeedleError_InvalidArgument, "downmix: channels must be 1 to " + std::to_string(NEEDLE_HIP_MAX_CHANNELS));
  if (pcm.size() != num_values.size() || out.size() != num_values.size())
    return Status::Make(NeedleError_InvalidArgument, "downmix: one length and one output per stream are required");
  Status s = ensure_device();
  if (!s.ok()) return s;
  // Batches of at most NEEDLE_HIP_MAX_BATCH_VALUES input values (2 GiB of s16 by default); a stream longer than that
  // is cut into pieces of whole 8-frame groups (frames are independent of each other).
  uint64_t max_values = 1ull << 30;
  if (const char *e = getenv("NEEDLE_HIP_MAX_BATCH_VALUES")) max_values = (uint64_t)std::max(1ll, atoll(e));  // tests
  const uint64_t C = (uint64_t)channels;
  const uint64_t piece_frames = std::max<uint64_t>(8, max_values / C / 8 * 8);
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
    uint64_t in_total = 0, out_total = 0;
    size_t end = begin;
    while (end < pieces.size() && (end == begin || in_total + pieces[end].frames * C <= max_values)) {
      pieces[end].in_off = in_total;
      pieces[end].out_off = out_total;
      in_total += (pieces[end].frames * C + 7) & ~(uint64_t)7;  // 16-byte aligned starts: the kernel's vector path
      out_total += (pieces[end].frames + 7) & ~(uint64_t)7;
      end++;
    }
    if (!(s = d_in.reserve(in_total)).ok() || !(s = d_out.reserve(out_total)).ok()) return s;
    std::vector<const int16_t *> src;
    std::vector<size_t> len;
    std::vector<uint64_t> off;
    std::vector<DownmixSpan> spans;
    for (size_t k = begin; k < end; k++) {
      const Piece &p = pieces[k];
      if (!pcm[p.stream] || !out[p.stream]) return Status::Make(NeedleError_NullArgument, "downmix: null stream pointer");
      src.push_back(pcm[p.stream] + p.first * C);
      len.push_back(p.frames * C);
      off.push_back(p.in_off);
      spans.push_back(DownmixSpan{d_in.ptr + p.in_off, d_out.ptr + p.out_off, p.frames});
    }
    s = gpu_upload_pcm(src, len, off, d_in.ptr, stream);
    if (s.ok()) s = gpu_downmix_device(spans, channels, false);
    // also on the error path: copies already enqueued read the caller's buffers asynchronously
    const bool drained = hipStreamSynchronize(stream) == hipSuccess;
    if (!s.ok()) return s;
    if (!drained) return Status::Make(NeedleError_Unknown, "downmix: upload or kernel failed");
    for (size_t k = begin; k < end; k++) {
      const Piece &p = pieces[k];
      NEEDLE_HIP_TRY(hipMemcpy(out[p.stream] + p.first, d_out.ptr + p.out_off, p.frames * sizeof(int16_t), hipMemcpyDeviceToHost));
    }
    begin = end;
  }
  return Status::Ok();
}

}  // namespace needle
