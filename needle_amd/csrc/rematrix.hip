// Channel mixes on the device: C-channel PCM in any sample format -> mono s16 through a layout-aware fold-down to stereo
// (include/needle_hip.h "Channel mixes").  Per frame, on the samples converted by to_s16:
//   acc_o = sum_c coef[o][c] * x_c   (Q15 coefficients, int32)      Lo, Ro = clip((acc_o + 16384) >> 15)
//   mono  = (Lo + Ro) / 2            (C division, the stereo path's rule)
// The host has checked sum_c |coef[o][c]| <= 65535, so |acc_o| <= 65535 * 32768 < 2^31 - 16384: nothing wraps.
//
// A streaming, memory-bound kernel in the mould of feeder_ingest_kernel (ingest_block.h): one launch over spans of any
// mixture of sample type, layout and channel count; virtual blocks of 256 lanes x 8 frames (16 of u8), grid stride, the
// span found by binary search; 16-byte loads and stores, unaligned sources and span tails on a scalar path.  A span's
// entry is the ingest's plus its 2 x 8 coefficients and a flag "plain average"; spans flagged plain run the shared
// ingest_block, so one launch lands a mixture of mixed and plain lanes.
//   * The entry is uniform over the workgroup, so the coefficients are scalar loads into SGPRs (both rows of a channel
//     lie side by side: one 8-byte load per channel).
//   * A lane keeps FPL pairs of int32 accumulators: registers do not grow with C.
//   * Both factors fit 24 bits (|coef| <= 32768, s16 samples): the products are v_mad_i32_i24, full rate, not the
//     quarter-rate 32-bit multiply.
#include "ingest_block.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>

namespace needle {

struct RematrixStream {
  IngestStream in;                           // what feeder_ingest_kernel's span holds
  int32_t coef[NEEDLE_HIP_MAX_CHANNELS][2];  // Q15: {to the left, to the right} of channel c
  int32_t plain;                             // no mix: (sum of the frame) / C, ingest_block
  int32_t pad;
};

namespace {

// coef * sample + acc with both factors inside 24 bits: one v_mad_i32_i24
__device__ __forceinline__ int mad24(int coef, int sample, int acc) { return __mul24(coef, sample) + acc; }

__device__ __forceinline__ int fold_down(int acc_l, int acc_r) {
  const int lo = min(max((acc_l + 16384) >> 15, -32768), 32767);
  const int ro = min(max((acc_r + 16384) >> 15, -32768), 32767);
  return (lo + ro) / 2;
}

template <typename T>
__device__ __forceinline__ void rematrix_block(const RematrixStream *__restrict__ rs, uint64_t block) {
  constexpr int FPL = frames_per_lane<T>();
  constexpr int NW = FPL / 2;  // output words of a lane, two s16 each
  const IngestStream *st = &rs->in;
  const uint64_t frames = st->frames;
  const uint64_t f0 = block * ((uint64_t)kCvThreads * FPL) + (uint64_t)threadIdx.x * FPL;
  if (f0 >= frames) return;
  const int C = st->channels;
  const bool planar = st->planar != 0;
  int16_t *y = st->dst + f0;
  if (f0 + FPL <= frames && st->vec) {
    uint32_t w[NW];
    if (planar) {
      constexpr int NV = FPL * (int)sizeof(T) / 16;
      int acc_l[FPL], acc_r[FPL];
#pragma unroll
      for (int f = 0; f < FPL; f++) acc_l[f] = acc_r[f] = 0;
      for (int c = 0; c < C; c++) {
        const int cl = rs->coef[c][0], cr = rs->coef[c][1];
        const uint4 *x = reinterpret_cast<const uint4 *>(static_cast<const T *>(st->src[c]) + f0);
        uint4 raw[NV];
#pragma unroll
        for (int k = 0; k < NV; k++) raw[k] = x[k];
        T p[FPL];
        __builtin_memcpy(p, raw, sizeof(raw));
#pragma unroll
        for (int f = 0; f < FPL; f++) {
          const int s = to_s16<T>(p[f]);
          acc_l[f] = mad24(cl, s, acc_l[f]);
          acc_r[f] = mad24(cr, s, acc_r[f]);
        }
      }
#pragma unroll
      for (int i = 0; i < NW; i++)
        w[i] = (uint32_t)(uint16_t)(int16_t)fold_down(acc_l[2 * i], acc_r[2 * i]) |
               ((uint32_t)(uint16_t)(int16_t)fold_down(acc_l[2 * i + 1], acc_r[2 * i + 1]) << 16);
    } else {
      constexpr int SPW = 16 / (int)sizeof(T);  // samples per 16-byte word
      const uint4 *x = reinterpret_cast<const uint4 *>(static_cast<const T *>(st->src[0]) + f0 * (uint64_t)C);
      const int words = C * (FPL / SPW);
#pragma unroll
      for (int i = 0; i < NW; i++) w[i] = 0;
      int acc_l = 0, acc_r = 0, ch = 0;
      for (int k = 0; k < words; k++) {
        const uint4 raw = x[k];
        T p[SPW];
        __builtin_memcpy(p, &raw, sizeof(raw));
#pragma unroll
        for (int e = 0; e < SPW; e++) {
          const int s = to_s16<T>(p[e]);
          acc_l = mad24(rs->coef[ch][0], s, acc_l);  // (ch is uniform over the workgroup: every lane starts at a frame)
          acc_r = mad24(rs->coef[ch][1], s, acc_r);
          if (++ch == C) {
            const uint32_t m = (uint32_t)(uint16_t)(int16_t)fold_down(acc_l, acc_r);
#pragma unroll
            for (int i = 0; i + 1 < NW; i++) w[i] = (w[i] >> 16) | (w[i + 1] << 16);
            w[NW - 1] = (w[NW - 1] >> 16) | (m << 16);
            acc_l = acc_r = 0;
            ch = 0;
          }
        }
      }
    }
    if ((reinterpret_cast<uintptr_t>(y) & 15) == 0) {
#pragma unroll
      for (int k = 0; k < NW / 4; k++)
        reinterpret_cast<uint4 *>(y)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    } else {
#pragma unroll
      for (int i = 0; i < NW; i++) {
        y[2 * i] = (int16_t)(w[i] & 0xFFFF);
        y[2 * i + 1] = (int16_t)(w[i] >> 16);
      }
    }
  } else {
    const int nf = frames - f0 < (uint64_t)FPL ? (int)(frames - f0) : FPL;
    for (int f = 0; f < nf; f++) {
      int acc_l = 0, acc_r = 0;
      for (int c = 0; c < C; c++) {
        const int s = to_s16<T>(planar ? static_cast<const T *>(st->src[c])[f0 + f] : static_cast<const T *>(st->src[0])[(f0 + f) * (uint64_t)C + c]);
        acc_l = mad24(rs->coef[c][0], s, acc_l);
        acc_r = mad24(rs->coef[c][1], s, acc_r);
      }
      y[f] = (int16_t)fold_down(acc_l, acc_r);
    }
  }
}

template <typename T>
__device__ __forceinline__ void land_block(const RematrixStream *__restrict__ rs, uint64_t block) {
  if (rs->plain) ingest_block<T>(&rs->in, block);
  else rematrix_block<T>(rs, block);
}

}  // namespace

// (a span's virtual blocks are of its own sample type's size: the table's block bases are counted on the host)
__global__ __launch_bounds__(kCvThreads) void rematrix_kernel(const RematrixStream *__restrict__ streams, int n, uint64_t blocks) {
  for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
    int lo = 0, hi = n - 1;  // last span whose block_base <= b (zero-frame spans are not in the table)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (streams[mid].in.block_base <= b) lo = mid;
      else hi = mid - 1;
    }
    const RematrixStream *rs = streams + lo;
    const uint64_t block = b - rs->in.block_base;
    switch (rs->in.type) {
      case NEEDLE_HIP_SAMPLE_U8: land_block<uint8_t>(rs, block); break;
      case NEEDLE_HIP_SAMPLE_S16: land_block<int16_t>(rs, block); break;
      case NEEDLE_HIP_SAMPLE_S32: land_block<int32_t>(rs, block); break;
      case NEEDLE_HIP_SAMPLE_F32: land_block<float>(rs, block); break;
      default: land_block<double>(rs, block); break;
    }
  }
}

Status gpu_rematrix_device(const std::vector<IngestSpan> &spans, bool sync) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s;
  for (const IngestSpan &sp : spans)  // before any device is asked for
    if (sp.mix && !(s = channel_mix_check(*sp.mix, sp.channels)).ok()) return s;
  if (!(s = ensure_device()).ok()) return s;
  int dev = 0;
  NEEDLE_HIP_TRY(hipGetDevice(&dev));
  std::vector<RematrixStream> meta;
  uint64_t blocks = 0;
  for (const IngestSpan &sp : spans) {
    RematrixStream rs{};
    if (!(s = ingest_stream_of(sp, &blocks, &rs.in)).ok()) return s;
    if (!rs.in.frames) continue;
    rs.plain = sp.mix == nullptr;
    for (int c = 0; sp.mix && c < sp.channels; c++) {
      rs.coef[c][0] = sp.mix->coef[0][c];
      rs.coef[c][1] = sp.mix->coef[1][c];
    }
    meta.push_back(rs);
  }
  if (meta.size() > 0x7FFFFFFFull) return Status::Make(NeedleError_InvalidArgument, "rematrix: too many spans for one launch");
  hipStream_t stream = library_stream();
  if (!meta.empty()) {
    // descriptor table: per device, pinned staging, in stream order behind the previous launch (as the ingest's)
    static std::map<int, std::pair<DeviceBuffer<RematrixStream> *, PinnedStage *>> ws;
    auto &w = ws[dev];
    if (!w.first) {
      w.first = new DeviceBuffer<RematrixStream>();
      w.second = new PinnedStage();
    }
    if (!(s = w.first->reserve(meta.size())).ok()) return s;
    if (!(s = w.second->acquire(meta.size() * sizeof(RematrixStream))).ok()) return s;
    std::memcpy(w.second->ptr, meta.data(), meta.size() * sizeof(RematrixStream));
    NEEDLE_HIP_TRY(hipMemcpyAsync(w.first->ptr, w.second->ptr, meta.size() * sizeof(RematrixStream), hipMemcpyHostToDevice, stream));
    w.second->mark(stream);
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(blocks, (uint64_t)std::max(cus, 1) * 8);  // the rest by grid stride
    KernelTimer timer("rematrix");
    hipLaunchKernelGGL(rematrix_kernel, dim3(grid), dim3(kCvThreads), 0, stream, w.first->ptr, (int)meta.size(), blocks);
    NEEDLE_HIP_TRY(hipGetLastError());
  }
  if (sync) NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  return Status::Ok();
}

}  // namespace needle
