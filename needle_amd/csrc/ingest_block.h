// What the landing kernels share (convert.hip, rematrix.hip): the per-sample conversion to s16 and the feeder's ingest of
// one virtual block of a span.  Device code, included by HIP translation units only.
#pragma once

#include <string>

#include "hipctx.h"

namespace needle {

namespace {

constexpr int kCvThreads = 256;

template <typename T>
__device__ __forceinline__ int to_s16(T x);
template <>
__device__ __forceinline__ int to_s16<uint8_t>(uint8_t x) {
  return ((int)x - 128) * 256;
}
template <>
__device__ __forceinline__ int to_s16<int16_t>(int16_t x) {
  return x;
}
template <>
__device__ __forceinline__ int to_s16<int32_t>(int32_t x) {
  return x >> 16;
}
template <>
__device__ __forceinline__ int to_s16<float>(float x) {
  const float y = rintf(x * 32768.0f);
  return y != y ? 0 : (int)fminf(fmaxf(y, -32768.0f), 32767.0f);  // clipped before the integer conversion
}
template <>
__device__ __forceinline__ int to_s16<double>(double x) {
  const double y = rint(x * 32768.0);
  return y != y ? 0 : (int)fmin(fmax(y, -32768.0), 32767.0);
}

template <typename T>
constexpr int frames_per_lane() {
  return sizeof(T) == 1 ? 16 : 8;
}

}  // namespace

// ---- the ingest of a feeder whose lanes have formats of their own ---------------------------------------------------
// One launch over spans of ANY mixture of sample type, layout and channel count, every one of them to mono s16:
// to_s16 per sample, then (sum of the frame's C values) / C on the int sum (C = 1: the conversion alone).  The mould
// is convert_kernel's -- virtual blocks of 256 lanes x 8 frames (16 of u8), grid stride, the span found by binary search
// -- but format and C are read from the span's entry, uniform over the workgroup: the sample type is switched over, C
// is a run-time loop.  A lane keeps FPL int sums at most, so the kernel's registers do not grow with C:
//   planar       plane after plane, FPL samples of each in 16-byte loads, added into the lane's FPL sums;
//   interleaved  the lane's FPL * C samples are C * FPL * sizeof(T) / 16 consecutive 16-byte words; their samples go by
//                in frame order, so one running sum and a channel counter do, and each finished frame is shifted
//                into the top of the lane's FPL / 2 output words (after FPL of them the first sits at the bottom).
// Sources that are not all 16-byte aligned (`vec` = 0, found on the host: a lane's first sample lies a multiple of 16
// bytes behind the span's) and the last frames of a span take the scalar path.
struct IngestStream {
  const void *src[NEEDLE_HIP_MAX_CHANNELS];  // planar: plane c; interleaved: src[0]
  int16_t *dst;
  uint64_t frames;
  uint64_t block_base;  // first virtual block of this span
  int32_t channels;
  int32_t type;    // format % 5
  int32_t planar;  // one plane per channel (and more than one channel)
  int32_t vec;     // every source pointer is 16-byte aligned
};

namespace {

// sum / C, C's division on the int sum, by a constant in every case: C is uniform over the workgroup, so the switch is
// one scalar branch and the divide a multiply-high and shifts instead of the emulated run-time division
__device__ __forceinline__ int div_channels(int sum, int C) {
  switch (C) {
    case 1: return sum;
    case 2: return sum / 2;
    case 3: return sum / 3;
    case 4: return sum / 4;
    case 5: return sum / 5;
    case 6: return sum / 6;
    case 7: return sum / 7;
    default: return sum / 8;
  }
}

template <typename T>
__device__ __forceinline__ void ingest_block(const IngestStream *__restrict__ st, uint64_t block) {
  constexpr int FPL = frames_per_lane<T>();
  constexpr int NW = FPL / 2;  // output words of a lane, two s16 each
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
      int sum[FPL];
#pragma unroll
      for (int f = 0; f < FPL; f++) sum[f] = 0;
      for (int c = 0; c < C; c++) {
        const uint4 *x = reinterpret_cast<const uint4 *>(static_cast<const T *>(st->src[c]) + f0);
        uint4 raw[NV];
#pragma unroll
        for (int k = 0; k < NV; k++) raw[k] = x[k];
        T p[FPL];
        __builtin_memcpy(p, raw, sizeof(raw));
#pragma unroll
        for (int f = 0; f < FPL; f++) sum[f] += to_s16<T>(p[f]);
      }
#pragma unroll
      for (int i = 0; i < NW; i++)
        w[i] = (uint32_t)(uint16_t)(int16_t)div_channels(sum[2 * i], C) | ((uint32_t)(uint16_t)(int16_t)div_channels(sum[2 * i + 1], C) << 16);
    } else {
      constexpr int SPW = 16 / (int)sizeof(T);  // samples per 16-byte word
      const uint4 *x = reinterpret_cast<const uint4 *>(static_cast<const T *>(st->src[0]) + f0 * (uint64_t)C);
      const int words = C * (FPL / SPW);
#pragma unroll
      for (int i = 0; i < NW; i++) w[i] = 0;
      int sum = 0, ch = 0;
      for (int k = 0; k < words; k++) {
        const uint4 raw = x[k];
        T p[SPW];
        __builtin_memcpy(p, &raw, sizeof(raw));
#pragma unroll
        for (int e = 0; e < SPW; e++) {
          sum += to_s16<T>(p[e]);
          if (++ch == C) {  // (uniform over the workgroup: every lane starts at a frame)
            const uint32_t m = (uint32_t)(uint16_t)(int16_t)div_channels(sum, C);
#pragma unroll
            for (int i = 0; i + 1 < NW; i++) w[i] = (w[i] >> 16) | (w[i + 1] << 16);
            w[NW - 1] = (w[NW - 1] >> 16) | (m << 16);
            sum = 0;
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
      int sum = 0;
      for (int c = 0; c < C; c++)
        sum += to_s16<T>(planar ? static_cast<const T *>(st->src[c])[f0 + f] : static_cast<const T *>(st->src[0])[(f0 + f) * (uint64_t)C + c]);
      y[f] = (int16_t)div_channels(sum, C);
    }
  }
}

}  // namespace

// host: the table entry of a span, its limits checked, behind `*blocks` virtual blocks (a span's blocks are of its own
// sample type's size).  A span without frames leaves out->frames 0 and is not put in the table.
inline Status ingest_stream_of(const IngestSpan &sp, uint64_t *blocks, IngestStream *out) {
  if (sp.channels < 1 || sp.channels > NEEDLE_HIP_MAX_CHANNELS)
    return Status::Make(NeedleError_InvalidArgument, "ingest: channels must be 1 to " + std::to_string(NEEDLE_HIP_MAX_CHANNELS));
  if (!sample_format_valid(sp.format)) return Status::Make(NeedleError_InvalidArgument, "ingest: unknown sample format");
  IngestStream st{};
  *out = st;
  if (sp.frames == 0) return Status::Ok();
  st.channels = sp.channels;
  st.type = sp.format % 5;
  st.planar = sample_format_planar(sp.format) && sp.channels > 1;
  uintptr_t align = 0;
  for (int c = 0; c < (st.planar ? sp.channels : 1); c++) {
    if (!sp.src[c]) return Status::Make(NeedleError_NullArgument, "ingest: null stream pointer");
    st.src[c] = sp.src[c];
    align |= reinterpret_cast<uintptr_t>(sp.src[c]);
  }
  if (!sp.dst) return Status::Make(NeedleError_NullArgument, "ingest: null stream pointer");
  st.vec = (align & 15) == 0;
  st.dst = sp.dst;
  st.frames = sp.frames;
  st.block_base = *blocks;
  const uint64_t block_frames = (uint64_t)kCvThreads * (sample_format_width(sp.format) == 1 ? 16 : 8);
  *blocks += (sp.frames + block_frames - 1) / block_frames;
  *out = st;
  return Status::Ok();
}

}  // namespace needle
