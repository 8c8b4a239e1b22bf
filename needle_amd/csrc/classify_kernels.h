// The fingerprinter's kernels behind the two transforms (stft_kernel.h, stft32_kernel.h), launched from fingerprint.hip:
//
//   features_classify : 5-tap temporal FIR {.25,.75,1,.75,.25} + L2 normalise (zero if norm < 0.01) into LDS,
//                       then 16 Haar-like filters over a 16x12 window, log-ratio quantised to 2 bits, Gray
//                       coded, packed MSB first -> u32 per kept item (items 0, step, 2*step, ...)
//   (fir_norm + classify: the same two steps as separate kernels, for callers that want the features)
//   features_classify_cert, fixup_items : the same over the f32 first pass's chroma, with the certificate, and the
//                       recomputation of the items it refuses
//   audit_items       : both pipelines side by side, item by item
//
// Included by fingerprint.hip alone: the kernels keep the names they have always had in traces and profiles,
// needle::(anonymous namespace)::, and are compiled in that unit with its flags.
#pragma once

#include "common.h"
#include "fp_core.h"
#include "stft32_kernel.h"  // kEnergyParts: the first pass's energy partials per frame
#include "stft_kernel.h"

namespace needle {
namespace {

using stft::FpStream;
using stft::find_stream;
using stft::stft_chroma_kernel;
using stft::wave_lds_fence;
using stft::kPairsPerBlock;

// One feature row: 5-tap temporal FIR over chroma rows in[0..4] + L2 normalise (zero if the norm is < 0.01).
__device__ __forceinline__ void feature_row(const double *__restrict__ in, double *out) {
  const double coef[5] = {0.25, 0.75, 1.0, 0.75, 0.25};
  double v[kBands];
  double squares = 0.0;
#pragma unroll
  for (int c = 0; c < kBands; c++) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 5; j++) acc += in[j * kBands + c] * coef[j];
    v[c] = acc;
    squares += acc * acc;
  }
  const double norm = squares > 0.0 ? sqrt(squares) : 0.0;
  if (norm < 0.01) {
#pragma unroll
    for (int c = 0; c < kBands; c++) out[c] = 0.0;
  } else {
#pragma unroll
    for (int c = 0; c < kBands; c++) out[c] = v[c] / norm;
  }
}

// ---- kernel 2: temporal FIR + L2 normalise, one thread per output row -------------------------------------
// (kernels 2 and 3 run separately only when a caller asks for the intermediate features; otherwise kernel 2+3)
__global__ __launch_bounds__(256) void fir_norm_kernel(const double *__restrict__ chroma,
                                                       const FpStream *__restrict__ streams, int num_streams,
                                                       double *__restrict__ feat, uint32_t total_rows) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total_rows) return;
  const int si = find_stream<&FpStream::fir_base>(streams, num_streams, g);
  const FpStream st = streams[si];
  const uint32_t r = g - st.fir_base;
  feature_row(chroma + ((uint64_t)st.frame_base + r) * kBands, feat + (uint64_t)g * kBands);
}

// ---- kernel 2+3: features of a tile in LDS, then its items -------------------------------------------------------
// A wave owns a tile of up to 64 consecutive kept items of one stream: it computes the (items - 1) step + 16
// feature rows the tile's windows cover into its own LDS region (each row once; neighbouring tiles repeat only the
// 15-row halo), then every lane classifies its window out of LDS.  The features never go to HBM and one dependent
// launch disappears.  Row pitch 13: with step 2 a lane's window starts 26 doubles after its neighbour's, which
// spreads the lanes over all banks (pitch 12 would put every fourth lane on the same ones).
constexpr int kTileRowsMax = 63 * 2 + 16;  // 64 items at the default step 2
constexpr int kFeatPitch = 13;
// PHASED (the feeder's classification table, gpu_fingerprint_feed_device): the stream's first kept item starts fir_base rows
// into its frames instead of at row 0 -- the carried region starts at an even frame, an item of an odd step need not.
template <bool PHASED = false>
__global__ __launch_bounds__(256) void features_classify_kernel(const double *__restrict__ chroma,
                                                                const FpStream *__restrict__ streams, int num_streams,
                                                                const core::ClassifierThresholds *__restrict__ thr,
                                                                uint32_t step, uint32_t items_per_tile,
                                                                uint32_t *__restrict__ items, uint32_t total_tiles) {
  __shared__ double tiles[4][kTileRowsMax * kFeatPitch];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t g = blockIdx.x * 4 + wave;
  if (g >= total_tiles) return;  // wave-uniform; the waves of a workgroup never wait for each other
  const int si = find_stream<&FpStream::tile_base>(streams, num_streams, g);
  const FpStream st = streams[si];
  const uint32_t k0 = (g - st.tile_base) * items_per_tile;
  const uint32_t count = min(items_per_tile, st.kept - k0);
  const uint32_t x0 = k0 * step + (PHASED ? st.fir_base : 0u);  // raw item index = first feature row of the tile
  const uint32_t rows = (count - 1) * step + 16;
  double *mine = tiles[wave];
  const double *in = chroma + ((uint64_t)st.frame_base + x0) * kBands;
  for (uint32_t r = lane; r < rows; r += 64) feature_row(in + (uint64_t)r * kBands, mine + r * kFeatPitch);
  wave_lds_fence();
  if (lane < count)
    items[st.item_off + k0 + lane] = core::classify_window<kFeatPitch>(mine + lane * step * kFeatPitch, thr);
}

// ---- certified first pass -----------------------------------------------------------------------------------------
// The chroma of stft_chroma32_kernel carries the f32 transform's error.  Measured with the kernel's own arithmetic
// stepped on the CPU (tools/f32_gate.py, profiles/r03_f32_gate.log): with v = (1 + a) / (1 + b) the input of a
// classifier,
//     |log v32 - log v64|  <=  1.8 * S,     S = max over the item's 16 feature rows of  u sqrt(E_row / n_row),
// u = 2^-24, n_row the row's L2 norm (what the features are divided by) and E_row its frames' total energy
// sum |X_k|^2 over ALL bins through the same 5-tap FIR -- on 28 x 24 min of synthetic episodes and on a zoo of signals
// that spans S from 1e-7 (tonal, in band) to 3e-4 (a strong tone outside chromaprint's band over a weak one inside).
// An item is ACCEPTED only if all 16 x 3 comparisons "v < exp(t)" clear their threshold by more than r = K S in
// log v (K = 64: 35 x the worst ratio observed) and none of its rows is within the same relative distance of the
// 0.01 norm cut; every other item (0.1 % of them on audio) is listed, the chunks of frame pairs its 20 frames span
// are listed once, stft_chroma_kernel<LISTED> overwrites those chroma rows in f64 and fixup_items_kernel recomputes
// the item from them with the arithmetic of features_classify_kernel.  So every emitted u32 is either certified to
// equal the f64 pipeline's or IS the f64 pipeline's.
struct CertItem {
  uint32_t row;   // chroma row of the item's first frame (global in the batch)
  uint32_t pad;
  uint64_t out;   // where its u32 goes in d_items
};
struct CertWork {      // zeroed before every batch (header + bitmap)
  uint32_t item_count, chunk_count, pad[2];
};
struct CertStats {     // cumulative, read by needle_hip_fingerprint_cert_stats
  unsigned long long items_recomputed, chunks_recomputed;
};
constexpr float kCertU = 5.9604644775390625e-08f;  // 2^-24
constexpr float kEnergyScale = 16384.0f;            // N * 4: the kernel's samples carry a factor 1/2 (fp_core.h)

// feature_row + the row's error scale sigma = u sqrt(E_row / n_row); +inf if the row sits within k sigma (relative) of
// the 0.01 cut, 0 if it is safely under it (features exactly zero in both pipelines) or silent.
// (T = float: a tile staged in LDS by features_classify_cert_kernel -- the first pass's chroma IS f32, kept as doubles in
// the buffer the f64 recomputation overwrites; the conversion back is exact and the row is the same bit for bit.)
template <typename T>
__device__ __forceinline__ float feature_row_cert(const T *__restrict__ in, const float *__restrict__ en, float k,
                                                  double *out) {
  const double coef[5] = {0.25, 0.75, 1.0, 0.75, 0.25};
  double v[kBands];
  double squares = 0.0;
#pragma unroll
  for (int c = 0; c < kBands; c++) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 5; j++) acc += (double)in[j * kBands + c] * coef[j];
    v[c] = acc;
    squares += acc * acc;
  }
  const double norm = squares > 0.0 ? sqrt(squares) : 0.0;
  float e_row = 0.0f;
#pragma unroll
  for (int j = 0; j < 5; j++)
    e_row += (float)coef[j] * ((en[j * stft::kEnergyParts] + en[j * stft::kEnergyParts + 1]) +
                               (en[j * stft::kEnergyParts + 2] + en[j * stft::kEnergyParts + 3]));
  float sigma = 0.0f;
  if (e_row > 0.0f) {
    const float n32 = fmaxf((float)norm, 1e-30f);
    sigma = kCertU * sqrtf(kEnergyScale * e_row / n32);
    if (fabsf(n32 - 0.01f) <= k * sigma * n32 + 1e-9f) sigma = __builtin_inff();
  }
  if (norm < 0.01) {
#pragma unroll
    for (int c = 0; c < kBands; c++) out[c] = 0.0;
    return sigma == __builtin_inff() ? sigma : 0.0f;
  }
  // one reciprocal instead of twelve divisions: a feature may differ from the f64 pipeline's by an ulp, 10^9 times less
  // than the radius an ACCEPTED item clears; every other item is recomputed by fixup_items_kernel with the divisions
  const double inv = 1.0 / norm;
#pragma unroll
  for (int c = 0; c < kBands; c++) out[c] = v[c] * inv;
  return sigma;
}

// classify_window + "is any of the 48 comparisons within rr (relative) of its threshold"
template <int PITCH, int ODD = 0>
__device__ __forceinline__ uint32_t classify_window_cert(const double *w, const core::ClassifierThresholds *thr, double rr,
                                                         bool *uncertain) {
  double a[16], b[16];
#pragma unroll
  for (int i = 0; i < 16; i++) a[i] = b[i] = 0.0;
  core::WindowStep<0, 0, PITCH, ODD>::run(w, a, b);
  uint32_t bits = 0;
  bool unc = false;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    // ratio < e^t  <=>  1 + a < e^t (1 + b)  (b >= 0): no division -- see feature_row_cert for why an ulp is harmless here
    const double num = 1.0 + a[i], den = 1.0 + b[i];
    const double d0 = thr->e[i][0] * den, d1 = thr->e[i][1] * den, d2 = thr->e[i][2] * den;
    const unsigned q = num < d1 ? (num < d0 ? 0u : 1u) : (num < d2 ? 2u : 3u);
    // |log ratio - t| <= r  <=  |ratio - e^t| <= e^t (r + r^2)  <=>  |num - e^t den| <= e^t den (r + r^2)   (rr = r + r^2, r < 1)
    unc = unc || fabs(num - d0) <= d0 * rr || fabs(num - d1) <= d1 * rr || fabs(num - d2) <= d2 * rr;
    bits = (bits << 2) | (q ^ (q >> 1));
  }
  *uncertain = unc;
  return bits;
}

// kCertWaves waves per workgroup, each with a tile of its own and no barrier between them: two, so that five workgroups
// (30 KB of LDS each) fit a CU -- the kernel is latency-bound and now needs 150 VGPRs, not 376 (fp_core.h WindowStep).
constexpr int kCertWaves = 2;
constexpr int kHalfRows = kTileRowsMax / 2;  // SPLIT: even rows of a tile first, its odd rows from here on
// SPLIT (chosen by the launcher when step == 2): the tile's rows lie de-interleaved in LDS (fp_core.h WindowStep ODD) --
// same values, same additions in the same order; only where a row is kept differs.
// PHASED: as in features_classify_kernel.  With SPLIT (a feed at step 2) the phase is even -- the tail starts at an even
// frame and the items of an even step at even frames -- so an item still starts at an even row of its tile.
template <bool SPLIT, bool PHASED = false>
__global__ __launch_bounds__(64 * kCertWaves) void features_classify_cert_kernel(
    const double *__restrict__ chroma, const float *__restrict__ energy, const FpStream *__restrict__ streams, int num_streams,
    const core::ClassifierThresholds *__restrict__ thr, uint32_t step, uint32_t items_per_tile, uint32_t *__restrict__ items,
    uint32_t total_tiles, float cert_k, uint32_t chunk_pairs, CertWork *__restrict__ work, uint32_t *__restrict__ chunk_bitmap,
    uint32_t *__restrict__ chunk_list, CertItem *__restrict__ item_list) {
  __shared__ double tiles[kCertWaves][kTileRowsMax * kFeatPitch];
  __shared__ float sigmas[kCertWaves][kTileRowsMax];
  // The tile's input -- rows + 4 chroma rows and their energy partials, one contiguous span each -- is staged first, with
  // coalesced 16-byte loads: every lane building its feature rows straight from global memory is 60 loads of 8 bytes at a
  // lane stride of 96 bytes, 48 cache lines per instruction, and the wave spent half its life waiting for them (SQ_WAIT_ANY
  // 49 % of SQ_WAVE_CYCLES, profiles/r04_final_summary.md).  The chroma is staged as the f32 it is (feature_row_cert).
  __shared__ __attribute__((aligned(16))) float stage[kCertWaves][(kTileRowsMax + 4) * kBands];
  __shared__ __attribute__((aligned(16))) float stage_en[kCertWaves][(kTileRowsMax + 4) * stft::kEnergyParts];
  static_assert(((kTileRowsMax + 4) * kBands) % 2 == 0 && stft::kEnergyParts == 4, "the staging loops move double2 / float4");
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t g = blockIdx.x * kCertWaves + wave;
  if (g >= total_tiles) return;  // wave-uniform; the waves of a workgroup never wait for each other
  __builtin_amdgcn_s_setprio(3);  // a tail kernel beside the next job's first pass: its waves issue first (fingerprint.hip, shared-CU overlap)
  const int si = find_stream<&FpStream::tile_base>(streams, num_streams, g);
  const FpStream st = streams[si];
  const uint32_t k0 = (g - st.tile_base) * items_per_tile;
  const uint32_t count = min(items_per_tile, st.kept - k0);
  const uint32_t x0 = k0 * step + (PHASED ? st.fir_base : 0u);
  const uint32_t rows = (count - 1) * step + 16;
  double *mine = tiles[wave];
  float *sig = sigmas[wave];
  const double *in = chroma + ((uint64_t)st.frame_base + x0) * kBands;
  const float *en = energy + ((uint64_t)st.frame_base + x0) * stft::kEnergyParts;
#ifdef NEEDLE_CERT_STAMPS
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  uint64_t t1 = 0, t2 = 0, t3 = 0;
#endif
  {
    float *sc = stage[wave], *se = stage_en[wave];
    const double2 *in2 = reinterpret_cast<const double2 *>(in);  // 96-byte rows: 16-byte aligned
    const float4 *en4 = reinterpret_cast<const float4 *>(en);
    const uint32_t n2 = (rows + 4) * kBands / 2, n4 = rows + 4;
    // every load of the tile in flight before the first is used (a rolled loop is one memory round trip per 1 KB:
    // 13 000 of the wave's 30 000 cycles when this was measured)
    constexpr int kLoads2 = ((kTileRowsMax + 4) * kBands / 2 + 63) / 64, kLoads4 = (kTileRowsMax + 4 + 63) / 64;
    double2 v2[kLoads2];
    float4 v4[kLoads4];
#pragma unroll
    for (int u = 0; u < kLoads2; u++) {
      const uint32_t i = lane + 64u * u;
      v2[u] = i < n2 ? in2[i] : double2{0.0, 0.0};
    }
#pragma unroll
    for (int u = 0; u < kLoads4; u++) {
      const uint32_t i = lane + 64u * u;
      v4[u] = i < n4 ? en4[i] : float4{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int u = 0; u < kLoads2; u++) {
      const uint32_t i = lane + 64u * u;
      if (i < n2) *reinterpret_cast<float2 *>(sc + 2 * i) = float2{(float)v2[u].x, (float)v2[u].y};
    }
#pragma unroll
    for (int u = 0; u < kLoads4; u++) {
      const uint32_t i = lane + 64u * u;
      if (i < n4) *reinterpret_cast<float4 *>(se + 4 * i) = v4[u];
    }
    wave_lds_fence();
#ifdef NEEDLE_CERT_STAMPS
    t1 = __builtin_amdgcn_s_memtime();
#endif
    for (uint32_t r = lane; r < rows; r += 64)
      sig[r] = feature_row_cert(sc + r * kBands, se + r * stft::kEnergyParts, cert_k,
                                mine + (SPLIT ? (r >> 1) + (r & 1u) * kHalfRows : r) * kFeatPitch);
  }
  wave_lds_fence();
#ifdef NEEDLE_CERT_STAMPS
  t2 = __builtin_amdgcn_s_memtime();
#endif
  if (lane < count) {
    float s_max = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; r++) s_max = fmaxf(s_max, sig[lane * step + r]);
    bool unc = false;
    const double r = (double)cert_k * (double)s_max;   // +inf when a row is at the norm cut
    const uint32_t bits = SPLIT ? classify_window_cert<kFeatPitch, kHalfRows * kFeatPitch>(mine + lane * kFeatPitch, thr, r + r * r, &unc)
                                : classify_window_cert<kFeatPitch>(mine + lane * step * kFeatPitch, thr, r + r * r, &unc);
    unc = unc || !(r < 0.25);                           // out of the calibrated regime: recompute
    const uint64_t out = st.item_off + k0 + lane;
    items[out] = bits;
#ifdef NEEDLE_CERT_STAMPS
    t3 = __builtin_amdgcn_s_memtime();
    if (lane == 0 && (g % 251) == 0)
      printf("cert tile %u rows %u: stage %llu, rows %llu, classify %llu cycles\n", g, rows, (unsigned long long)(t1 - t0),
             (unsigned long long)(t2 - t1), (unsigned long long)(t3 - t2));
#endif
    if (unc) {
      const uint32_t x = x0 + lane * step;              // raw item = first frame of the 20 it covers
      item_list[atomicAdd(&work->item_count, 1u)] = CertItem{st.frame_base + x, 0u, out};
      const uint32_t p0 = st.pair_base + x / 2, p1 = st.pair_base + min(x + 19u, st.frames - 1u) / 2;
      for (uint32_t c = p0 / chunk_pairs; c <= p1 / chunk_pairs; c++) {
        const uint32_t bit = 1u << (c & 31u);
        if (!(atomicOr(&chunk_bitmap[c >> 5], bit) & bit)) chunk_list[atomicAdd(&work->chunk_count, 1u)] = c;
      }
    }
  }
}

// one wave per listed item: its 16 feature rows from the (now f64) chroma rows, then the 16 classifiers -- the
// arithmetic of features_classify_kernel, function for function
__global__ __launch_bounds__(256) void fixup_items_kernel(const double *__restrict__ chroma,
                                                          const core::ClassifierThresholds *__restrict__ thr,
                                                          const CertWork *__restrict__ work, const CertItem *__restrict__ item_list,
                                                          uint32_t *__restrict__ items, CertStats *__restrict__ stats,
                                                          uint32_t *__restrict__ zero_word) {
  __shared__ double tiles[4][16 * kFeatPitch];
  __builtin_amdgcn_s_setprio(3);  // a tail kernel beside the next job's first pass: its waves issue first (fingerprint.hip, shared-CU overlap)
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t n = work->item_count;
  double *mine = tiles[wave];
  for (uint32_t i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
    const CertItem it = item_list[i];
    if (lane < 16) feature_row(chroma + ((uint64_t)it.row + lane) * kBands, mine + lane * kFeatPitch);
    wave_lds_fence();
    if (lane == 0) items[it.out] = core::classify_window<kFeatPitch>(mine, thr);
    wave_lds_fence();  // the next item of this wave overwrites the tile
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (zero_word) *zero_word = 0u;  // the run counter of the scan that follows (a memset dispatch less in front of it)
    atomicAdd(&stats->items_recomputed, (unsigned long long)n);
    atomicAdd(&stats->chunks_recomputed, (unsigned long long)work->chunk_count);
  }
}

// ---- audit of the certified first pass -----------------------------------------------------------------------------
// Not part of a job: needle_hip_fingerprint_audit_device / needle_hip_library_audit run BOTH transforms over the same
// resident PCM -- stft_chroma32_kernel into one chroma buffer, stft_chroma_kernel (f64) into another -- and this kernel
// then looks at every kept item with the certification kernel's own functions: the acceptance decision from the f32
// chroma (feature_row_cert, classify_window_cert, the same K), the f64 pipeline's item from the f64 chroma
// (feature_row, classify_window), and for every ACCEPTED item the quantity the radius is a bound on,
//     max over the 16 classifiers of |log v32 - log v64| / S,      v = (1 + a) / (1 + b),
// reduced to a maximum over the batch.  Counts: accepted items whose f32 bits differ from the f64 item (each one a
// hole in the guarantee: must be 0), and items of the product's own output `items` that differ from the f64 item.
struct AuditCounts {
  unsigned long long items, accepted, accepted_wrong, final_wrong;
  unsigned long long max_ratio_bits, max_sigma_bits;  // doubles >= 0 compare like their bit patterns
};
// PHASED (an audited feed, gpu_fingerprint_feed_device): as in features_classify_cert_kernel, over the feed's `second`
// table -- chroma32 / energy the feeder's first-pass rows, chroma64 the audit's own, `items` the round's.  `out` is then
// one AuditCounts per feeder lane, and stream si of the table counts into out[lane_of[si]], lane_of the u32 array that
// lies right behind the table's last stream (it travels with the table's upload).
template <bool PHASED = false>
__global__ __launch_bounds__(64) void audit_items_kernel(const double *__restrict__ chroma32, const float *__restrict__ energy,
                                                         const double *__restrict__ chroma64, const FpStream *__restrict__ streams,
                                                         int num_streams, const core::ClassifierThresholds *__restrict__ thr,
                                                         uint32_t step, uint32_t items_per_tile, const uint32_t *__restrict__ items,
                                                         uint32_t total_tiles, float cert_k, AuditCounts *__restrict__ out) {
  __shared__ double tile32[kTileRowsMax * kFeatPitch], tile64[kTileRowsMax * kFeatPitch];
  __shared__ float sig[kTileRowsMax];
  const uint32_t lane = threadIdx.x, g = blockIdx.x;
  if (g >= total_tiles) return;
  const int si = find_stream<&FpStream::tile_base>(streams, num_streams, g);
  const FpStream st = streams[si];
  const uint32_t k0 = (g - st.tile_base) * items_per_tile;
  const uint32_t count = min(items_per_tile, st.kept - k0);
  const uint32_t x0 = k0 * step + (PHASED ? st.fir_base : 0u);
  const uint32_t rows = (count - 1) * step + 16;
  const uint64_t row0 = (uint64_t)st.frame_base + x0;
  if (PHASED) out += reinterpret_cast<const uint32_t *>(streams + num_streams)[si];
  for (uint32_t r = lane; r < rows; r += 64) {
    sig[r] = feature_row_cert(chroma32 + (row0 + r) * kBands, energy + (row0 + r) * stft::kEnergyParts, cert_k, tile32 + r * kFeatPitch);
    feature_row(chroma64 + (row0 + r) * kBands, tile64 + r * kFeatPitch);
  }
  wave_lds_fence();
  if (lane >= count) return;
  float s_max = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; r++) s_max = fmaxf(s_max, sig[lane * step + r]);
  bool unc = false;
  const double r = (double)cert_k * (double)s_max;
  const uint32_t bits32 = classify_window_cert<kFeatPitch>(tile32 + lane * step * kFeatPitch, thr, r + r * r, &unc);
  unc = unc || !(r < 0.25);
  const uint32_t bits64 = core::classify_window<kFeatPitch>(tile64 + lane * step * kFeatPitch, thr);
  atomicAdd(&out->items, 1ull);
  if (items[st.item_off + k0 + lane] != bits64) atomicAdd(&out->final_wrong, 1ull);
  if (unc) return;
  atomicAdd(&out->accepted, 1ull);
  if (bits32 != bits64) atomicAdd(&out->accepted_wrong, 1ull);
  double a32[16], b32[16], a64[16], b64[16];
#pragma unroll
  for (int i = 0; i < 16; i++) a32[i] = b32[i] = a64[i] = b64[i] = 0.0;
  core::WindowStep<0, 0, kFeatPitch>::run(tile32 + lane * step * kFeatPitch, a32, b32);
  core::WindowStep<0, 0, kFeatPitch>::run(tile64 + lane * step * kFeatPitch, a64, b64);
  double err = 0.0;
#pragma unroll
  for (int i = 0; i < 16; i++)
    err = fmax(err, fabs(log((1.0 + a32[i]) / (1.0 + b32[i])) - log((1.0 + a64[i]) / (1.0 + b64[i]))));
  // S = 0: silence or rows under the norm cut in both pipelines -- every feature is exactly zero, err must be too
  const double ratio = s_max > 0.0f ? err / (double)s_max : (err > 0.0 ? __builtin_inf() : 0.0);
  atomicMax(&out->max_ratio_bits, (unsigned long long)__double_as_longlong(ratio));
  atomicMax(&out->max_sigma_bits, (unsigned long long)__double_as_longlong((double)s_max));
}

// ---- kernel 3: 16 classifiers over a 16x12 window, one thread per kept item ----------------------------------
__global__ __launch_bounds__(256) void classify_kernel(const double *__restrict__ feat,
                                                       const FpStream *__restrict__ streams, int num_streams,
                                                       const core::ClassifierThresholds *__restrict__ thr,
                                                       uint32_t step, uint32_t *__restrict__ items,
                                                       uint32_t total_kept) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total_kept) return;
  const int si = find_stream<&FpStream::kept_base>(streams, num_streams, g);
  const FpStream st = streams[si];
  const uint32_t k = g - st.kept_base;
  const uint32_t x = k * step;  // raw item index = first row of the window
  const double *w = feat + ((uint64_t)st.fir_base + x) * kBands;
  const uint32_t bits = core::classify_window(w, thr);
  items[st.item_off + k] = bits;
}

}  // namespace
}  // namespace needle
