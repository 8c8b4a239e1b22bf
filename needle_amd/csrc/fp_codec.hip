// chromaprint's fingerprint codec on the device, batched: many fingerprints per call, concatenated, with an offsets row.
// The format and every expression that decides what a lane reads or writes are in fp_codec.h; DESIGN.md 4e has the
// passes, the resources and the limits.
//
// Compress (tiles of kFpcTileItems items, never across two fingerprints; a lane takes 4 consecutive items):
//   fp_compress_count   per tile: symbols and exceptional symbols of its items
//   fp_compress_layout  one workgroup: per fingerprint the exclusive scan of its tiles' counts, S, E and the blob's size;
//                       then the exclusive scan of the sizes = where each blob starts.  Nothing is downloaded.
//   fp_compress_zero    zeroes the bytes the layout found (the total is read on the device)
//   fp_compress_pack    per tile: the scan of the counts inside the tile, the tile's bits of both streams assembled in
//                       LDS (atomic OR of each item's shifted symbols), whole aligned words stored coalesced; the words
//                       at the ends of the tile's span, which a neighbour may share, are ORed into the zeroed output.
// Decompress (tiles of kFpdTileSymbols 3-bit symbols over everything behind a blob's header; a lane takes 8 = 3 bytes):
//   fp_decompress_count   per tile: zeros (terminators) and sevens
//   fp_decompress_layout  one workgroup per blob: the exclusive scan of its tiles' counts, the tile that holds the n-th
//                         zero, in it S and E, and the refusals 2 and 3
//   fp_decompress_unpack  per tile: scans of the zero flags (symbol -> item) and of the seven flags (-> exceptional
//                         index), the segmented sum of the gaps inside an item (-> bit position; the tile's first item
//                         takes its start from fpd_tile_carry), the bits ORed into the item's delta; refusal 4 is flagged
//   fp_decompress_xor     one workgroup per fingerprint: refusal 4 where flagged, else the inclusive XOR-scan of its deltas, in place
#include "fp_codec.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "hipctx.h"

namespace needle {

// ---- workgroup scans: wave64 scans by lane shuffles (DPP row shifts and a permute across rows), the four waves' totals
// through LDS.  op(earlier, later); `tot`: 4 words of LDS.  Every lane of the workgroup calls. -------------------------
template <class Op>
__device__ inline void block_scan(uint32_t v, Op op, uint32_t identity, uint32_t *tot, uint32_t *incl, uint32_t *excl, uint32_t *total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d, 64);
    if (lane >= d) v = op(o, v);
  }
  uint32_t before = __shfl_up(v, 1, 64);
  if (lane == 0) before = identity;
  __syncthreads();  // the previous scan's totals have been read
  if (lane == 63) tot[wave] = v;
  __syncthreads();
  uint32_t pre = identity;
  for (uint32_t k = 0; k < wave; k++) pre = op(pre, tot[k]);
  if (incl) *incl = op(pre, v);
  if (excl) *excl = op(pre, before);
  if (total) *total = op(op(op(tot[0], tot[1]), tot[2]), tot[3]);
}
struct AddOp {
  __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
struct XorOp {
  __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a ^ b; }
};
// segmented sum: bit 31 = "a terminator lies in the range", bits 0..30 = the gaps behind the last terminator of the range
struct SegOp {
  __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return fpd_seg_combine(a, b); }
};

// ORs byte `value` into out[at] of a zeroed buffer: an atomic OR on the aligned word around it
__device__ inline void or_byte(uint8_t *out, uint64_t at, uint32_t value) {
  uint8_t *p = out + at;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (value) atomicOr(reinterpret_cast<uint32_t *>(a & ~(uintptr_t)3), value << (8 * (a & 3)));
}

// ---- compress ------------------------------------------------------------------------------------------------------
struct FpcBatch {
  const uint32_t *items;      // concatenated
  const uint32_t *item_off;   // count + 1
  const uint32_t *tile_base;  // count + 1: fingerprint b owns tiles [tile_base[b], tile_base[b + 1])
  uint32_t count, tiles;
  uint32_t *tile_sym, *tile_exc;        // per tile: its counts, then (layout) the counts of the fingerprint's earlier tiles
  uint32_t *fp_sym, *fp_exc;            // per fingerprint: S and E
  uint32_t *blob_off;                   // count + 1
  uint8_t *out;
  uint32_t out_capacity;                // bytes, a multiple of 4
  uint32_t algorithm;
};

// the lane's 4 deltas in tile `tile_in_fp` of fingerprint b
__device__ inline uint32_t lane_deltas(const FpcBatch &q, uint32_t b, uint32_t tile_in_fp, uint32_t x[kFpcLaneItems]) {
  const uint32_t lo = q.item_off[b];
  return fpc_lane_deltas(q.items + lo, q.item_off[b + 1] - lo, tile_in_fp, threadIdx.x, x);
}

__global__ __launch_bounds__(kFpcThreads) void fp_compress_count_kernel(FpcBatch q) {
  __shared__ uint32_t tot[4];
  for (uint32_t t = blockIdx.x; t < q.tiles; t += gridDim.x) {
    const uint32_t b = fpc_tile_owner(q.tile_base, q.count, t);
    uint32_t x[kFpcLaneItems];
    const uint32_t have = lane_deltas(q, b, t - q.tile_base[b], x);
    uint32_t packed = 0;  // symbols (at most 33 * 1024) | exceptional (at most 4 * 1024) << 16
    for (uint32_t k = 0; k < have; k++) {
      const FpcItemBits bits = fpc_item_bits(x[k]);
      packed += bits.nsym | (bits.nexc << 16);
    }
    uint32_t total;
    block_scan(packed, AddOp(), 0, tot, nullptr, nullptr, &total);
    if (threadIdx.x == 0) {
      q.tile_sym[t] = total & 0xFFFF;
      q.tile_exc[t] = total >> 16;
    }
  }
}

__global__ __launch_bounds__(kFpcThreads) void fp_compress_layout_kernel(FpcBatch q) {
  __shared__ uint32_t tot[4];
  // per fingerprint (a lane each): its tiles' counts -> exclusive prefixes, S, E, the blob's size into blob_off[b + 1]
  for (uint32_t b = threadIdx.x; b < q.count; b += kFpcThreads) {
    uint32_t s = 0, e = 0;
    for (uint32_t t = q.tile_base[b]; t < q.tile_base[b + 1]; t++) {
      const uint32_t ts = q.tile_sym[t], te = q.tile_exc[t];
      q.tile_sym[t] = s;
      q.tile_exc[t] = e;
      s += ts;
      e += te;
    }
    q.fp_sym[b] = s;
    q.fp_exc[b] = e;
    q.blob_off[b + 1] = (uint32_t)fpc_blob_bytes(s, e);
  }
  __syncthreads();
  // the exclusive scan of the sizes, 256 fingerprints at a time
  uint32_t carry = 0;
  for (uint32_t base = 0; base < q.count; base += kFpcThreads) {
    const uint32_t b = base + threadIdx.x;
    const uint32_t size = b < q.count ? q.blob_off[b + 1] : 0;
    uint32_t incl, total;
    block_scan(size, AddOp(), 0, tot, &incl, nullptr, &total);
    if (b < q.count) q.blob_off[b + 1] = carry + incl;
    carry += total;
  }
  if (threadIdx.x == 0) q.blob_off[0] = 0;
}

__global__ __launch_bounds__(kFpcThreads) void fp_compress_zero_kernel(FpcBatch q) {
  const uint32_t words = std::min((q.blob_off[q.count] + 3) / 4, q.out_capacity / 4);
  uint32_t *out = reinterpret_cast<uint32_t *>(q.out);
  for (uint32_t w = blockIdx.x * kFpcThreads + threadIdx.x; w < words; w += gridDim.x * kFpcThreads) out[w] = 0;
}

// a tile's assembled bytes -> the output: whole words stored where the tile owns them, ORed otherwise (fp_codec.h)
__device__ inline void store_span(const uint32_t *lds, const FpcSpan &span, uint8_t *out, uint64_t stream_at, uint64_t limit) {
  fpc_store_span_lane(
      reinterpret_cast<const uint8_t *>(lds), span, stream_at, limit, threadIdx.x,
      [&](uint64_t word, uint32_t value) { *reinterpret_cast<uint32_t *>(out + word) = value; },  // (the output's base is word-aligned)
      [&](uint64_t word, uint32_t value) { atomicOr(reinterpret_cast<uint32_t *>(out + word), value); });
}

__global__ __launch_bounds__(kFpcThreads) void fp_compress_pack_kernel(FpcBatch q) {
  __shared__ uint32_t tot[4];
  __shared__ uint32_t normal[kFpcNormalWords];
  __shared__ uint32_t exceptional[kFpcExceptionalWords];
  for (uint32_t t = blockIdx.x; t < q.tiles; t += gridDim.x) {
    const uint32_t b = fpc_tile_owner(q.tile_base, q.count, t);
    const uint32_t tile_in_fp = t - q.tile_base[b];
    const uint64_t blob_at = q.blob_off[b], blob_end = std::min(q.blob_off[b + 1], q.out_capacity);
    uint32_t x[kFpcLaneItems];
    const uint32_t have = lane_deltas(q, b, tile_in_fp, x);
    FpcItemBits bits[kFpcLaneItems];
    uint32_t packed = 0;
#pragma unroll
    for (uint32_t k = 0; k < kFpcLaneItems; k++) {
      bits[k] = fpc_item_bits(x[k]);
      if (k < have) packed += bits[k].nsym | (bits[k].nexc << 16);
    }
    for (uint32_t w = threadIdx.x; w < kFpcNormalWords; w += kFpcThreads) normal[w] = 0;
    for (uint32_t w = threadIdx.x; w < kFpcExceptionalWords; w += kFpcThreads) exceptional[w] = 0;
    uint32_t excl, total;
    block_scan(packed, AddOp(), 0, tot, nullptr, &excl, &total);  // (its barriers also publish the zeroed buffers)
    const uint32_t sym0 = q.tile_sym[t], exc0 = q.tile_exc[t];    // symbols of the fingerprint's earlier tiles
    const FpcSpan ns = fpc_tile_span(sym0, total & 0xFFFF, 3), es = fpc_tile_span(exc0, total >> 16, 5);
    uint32_t s = excl & 0xFFFF, e = excl >> 16;  // symbols of the tile's earlier items
#pragma unroll
    for (uint32_t k = 0; k < kFpcLaneItems; k++) {
      if (k >= have) continue;
      fpc_place_bits(ns.lead_bits + 3 * s, bits[k].lo, bits[k].hi, kFpcNormalWords, [&](uint32_t w, uint32_t v) { atomicOr(&normal[w], v); });
      fpc_place_bits(es.lead_bits + 5 * e, bits[k].exc, 0, kFpcExceptionalWords, [&](uint32_t w, uint32_t v) { atomicOr(&exceptional[w], v); });
      s += bits[k].nsym;
      e += bits[k].nexc;
    }
    __syncthreads();
    store_span(normal, ns, q.out, blob_at + fpc_normal_start(), blob_end);
    store_span(exceptional, es, q.out, blob_at + fpc_exceptional_start(q.fp_sym[b]), blob_end);
    if (tile_in_fp == 0 && threadIdx.x < kFpcHeaderBytes && blob_at + threadIdx.x < blob_end) {
      const uint32_t n = q.item_off[b + 1] - q.item_off[b];
      const uint32_t header[kFpcHeaderBytes] = {q.algorithm & 0xFF, (n >> 16) & 0xFF, (n >> 8) & 0xFF, n & 0xFF};
      or_byte(q.out, blob_at + threadIdx.x, header[threadIdx.x]);
    }
    __syncthreads();  // the buffers are zeroed again for the next tile
  }
}

// ---- decompress ----------------------------------------------------------------------------------------------------
struct FpdBatch {
  const uint8_t *blobs;       // concatenated
  const uint32_t *blob_off;   // count + 1
  const uint32_t *tile_base;  // count + 1: tiles over fpc_max_symbols(bytes) symbols; a blob without symbols has one
  const uint32_t *items_n;    // per blob: the header's n where the host accepted it (the slot's size), else 0
  const uint32_t *slot_off;   // count + 1
  uint32_t count, tiles;
  uint32_t *tile_zero, *tile_seven;  // per tile: its counts, then (layout) the counts of the blob's earlier tiles
  uint32_t *fp_sym, *fp_exc;         // per blob: S and E
  int32_t *status;                   // per blob; the host's verdict on the way in
  uint32_t *bad;                     // per blob, zeroed: unpack found a bit position above 32 (status stays as it is while
                                     // unpack runs, so that every lane of a workgroup reads the same; xor moves it over)
  uint32_t *out;                     // deltas, then items
};

__global__ __launch_bounds__(kFpcThreads) void fp_decompress_count_kernel(FpdBatch q) {
  __shared__ uint32_t tot[4];
  for (uint32_t t = blockIdx.x; t < q.tiles; t += gridDim.x) {
    const uint32_t b = fpc_tile_owner(q.tile_base, q.count, t);
    const uint64_t bytes = q.blob_off[b + 1] - q.blob_off[b];
    uint32_t valid, zeros, sevens, total = 0;
    if (q.status[b] == kFpcOk) {  // (uniform: a refused blob's tile counts nothing)
      fpd_lane_symbols(q.blobs + q.blob_off[b], bytes, (uint64_t)(t - q.tile_base[b]) * kFpdTileSymbols, fpc_max_symbols(bytes), threadIdx.x,
                       &valid, &zeros, &sevens);
      block_scan(zeros | (sevens << 16), AddOp(), 0, tot, nullptr, nullptr, &total);  // at most 2048 each
    }
    if (threadIdx.x == 0) {
      q.tile_zero[t] = total & 0xFFFF;
      q.tile_seven[t] = total >> 16;
    }
  }
}

__global__ __launch_bounds__(kFpcThreads) void fp_decompress_layout_kernel(FpdBatch q) {
  __shared__ uint32_t tot[4];
  __shared__ uint32_t found[4];  // {tile, zeros before it, sevens before it, found}; then {S, E, found}
  for (uint32_t b = blockIdx.x; b < q.count; b += gridDim.x) {
    __syncthreads();  // `found` of the previous blob has been read
    if (threadIdx.x == 0) {
      found[3] = 0;
      q.fp_sym[b] = 0;
      q.fp_exc[b] = 0;
    }
    const uint32_t n = q.items_n[b];
    if (q.status[b] != kFpcOk || n == 0) continue;  // uniform.  n = 0: S = E = 0, whatever follows the header
    const uint32_t t0 = q.tile_base[b], t1 = q.tile_base[b + 1];
    uint32_t zeros_before = 0, sevens_before = 0;
    for (uint32_t base = t0; base < t1; base += kFpcThreads) {
      const uint32_t t = base + threadIdx.x;
      const uint32_t z = t < t1 ? q.tile_zero[t] : 0, s = t < t1 ? q.tile_seven[t] : 0;
      uint32_t zi, ze, zt, si_unused, se, st;
      block_scan(z, AddOp(), 0, tot, &zi, &ze, &zt);
      block_scan(s, AddOp(), 0, tot, &si_unused, &se, &st);
      if (t < t1) {
        q.tile_zero[t] = zeros_before + ze;
        q.tile_seven[t] = sevens_before + se;
        if (zeros_before + ze < n && zeros_before + zi >= n) {  // the tile of the n-th zero: one lane at most
          found[0] = t;
          found[1] = zeros_before + ze;
          found[2] = sevens_before + se;
          found[3] = 1;
        }
      }
      zeros_before += zt;
      sevens_before += st;
      __syncthreads();
      if (found[3]) break;  // uniform
    }
    if (!found[3]) {
      if (threadIdx.x == 0) q.status[b] = kFpcNormalEnds;
      continue;
    }
    // inside that tile: the (n - zeros before it)-th zero ends the normal stream
    const uint32_t t = found[0], want = n - found[1], tile_sevens = found[2];
    const uint64_t bytes = q.blob_off[b + 1] - q.blob_off[b];
    const uint64_t first = (uint64_t)(t - t0) * kFpdTileSymbols;
    uint32_t valid, zeros, sevens, excl;
    const uint32_t v = fpd_lane_symbols(q.blobs + q.blob_off[b], bytes, first, fpc_max_symbols(bytes), threadIdx.x, &valid, &zeros, &sevens);
    block_scan(zeros | (sevens << 16), AddOp(), 0, tot, nullptr, &excl, nullptr);  // (its barriers: found[] has been read)
    uint32_t in_tile, sevens_in_tile;
    if (fpd_lane_locate(v, valid, threadIdx.x, excl & 0xFFFF, excl >> 16, want, &in_tile, &sevens_in_tile)) {  // one lane
      const uint64_t S = first + in_tile, E = (uint64_t)tile_sevens + sevens_in_tile;
      q.fp_sym[b] = (uint32_t)S;
      q.fp_exc[b] = (uint32_t)E;
      if (fpc_blob_bytes(S, E) > bytes) q.status[b] = kFpcExceptionalEnds;
    }
  }
}

__global__ __launch_bounds__(kFpcThreads) void fp_decompress_unpack_kernel(FpdBatch q) {
  __shared__ uint32_t tot[4];
  __shared__ uint32_t carry;
  for (uint32_t t = blockIdx.x; t < q.tiles; t += gridDim.x) {
    const uint32_t b = fpc_tile_owner(q.tile_base, q.count, t);
    const uint64_t S = q.fp_sym[b], first = (uint64_t)(t - q.tile_base[b]) * kFpdTileSymbols;
    if (q.status[b] != kFpcOk || first >= S) continue;  // uniform
    const uint8_t *blob = q.blobs + q.blob_off[b];
    const uint64_t bytes = q.blob_off[b + 1] - q.blob_off[b], exc_start = fpc_exceptional_start(S);
    const uint32_t n = q.items_n[b], zeros_before = q.tile_zero[t], sevens_before = q.tile_seven[t];
    __syncthreads();  // `carry` of the previous tile has been read
    if (threadIdx.x == 0) carry = fpd_tile_carry(blob, bytes, exc_start, first, sevens_before);
    uint32_t valid, zeros, sevens, counts;
    const uint32_t v = fpd_lane_symbols(blob, bytes, first, S, threadIdx.x, &valid, &zeros, &sevens);
    block_scan(zeros | (sevens << 16), AddOp(), 0, tot, nullptr, &counts, nullptr);
    uint32_t gap[kFpdLaneSymbols];
    const uint32_t seg = fpd_lane_gaps(blob, bytes, exc_start, v, valid, (uint64_t)sevens_before + (counts >> 16), gap);
    uint32_t before;
    block_scan(seg, SegOp(), 0, tot, nullptr, &before, nullptr);  // (its barriers publish `carry`)
    const uint32_t pos = (before & 0x7FFFFFFFu) + ((before >> 31) ? 0 : carry);
    uint32_t *slot = q.out + q.slot_off[b];
    const bool good = fpd_lane_emit(gap, valid, zeros_before + (counts & 0xFFFF), pos, n, [&](uint32_t item, uint32_t bits) { atomicOr(&slot[item], bits); });
    if (!good) atomicOr(&q.bad[b], 1u);
  }
}

__global__ __launch_bounds__(kFpcThreads) void fp_decompress_xor_kernel(FpdBatch q) {
  __shared__ uint32_t tot[4];
  for (uint32_t b = blockIdx.x; b < q.count; b += gridDim.x) {
    if (q.status[b] != kFpcOk) continue;  // uniform
    if (q.bad[b]) {                       // uniform
      if (threadIdx.x == 0) q.status[b] = kFpcBitPosition;
      continue;
    }
    uint32_t *slot = q.out + q.slot_off[b];
    const uint32_t n = std::min(q.items_n[b], q.slot_off[b + 1] - q.slot_off[b]);
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += kFpcTileItems) {
      const uint32_t i0 = base + threadIdx.x * kFpcLaneItems;
      uint32_t x[kFpcLaneItems], mine = 0;
#pragma unroll
      for (uint32_t k = 0; k < kFpcLaneItems; k++) {
        x[k] = i0 + k < n ? slot[i0 + k] : 0;
        mine ^= x[k];
      }
      uint32_t before, total;
      block_scan(mine, XorOp(), 0, tot, nullptr, &before, &total);
      uint32_t run = carry ^ before;
#pragma unroll
      for (uint32_t k = 0; k < kFpcLaneItems; k++) {
        run ^= x[k];
        if (i0 + k < n) slot[i0 + k] = run;
      }
      carry ^= total;
    }
  }
}

// ---- host drivers --------------------------------------------------------------------------------------------------
namespace {

uint32_t grid_for(uint64_t blocks) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)device_cu_count() * 8));  // the rest by grid stride
}

template <class T>
Status upload(DeviceBuffer<T> *dst, const std::vector<T> &src, hipStream_t stream) {
  Status s = dst->reserve(std::max<size_t>(src.size(), 1));
  if (!s.ok()) return s;
  if (!src.empty()) NEEDLE_HIP_TRY(hipMemcpyAsync(dst->ptr, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, stream));
  return Status::Ok();
}

// fingerprints [b0, b1) of the call: one launch chain
Status compress_batch(const uint32_t *items, const uint64_t *item_off, size_t b0, size_t b1, int algorithm, std::vector<uint8_t> *blobs,
                      std::vector<uint64_t> *blob_off) {
  const uint32_t count = (uint32_t)(b1 - b0);
  const uint64_t total_items = item_off[b1] - item_off[b0];
  std::vector<uint32_t> off(count + 1), tile_base(count + 1);
  uint64_t tiles = 0, capacity = 0;
  for (uint32_t b = 0; b <= count; b++) {
    off[b] = (uint32_t)(item_off[b0 + b] - item_off[b0]);
    tile_base[b] = (uint32_t)tiles;
    if (b < count) {
      const uint64_t n = item_off[b0 + b + 1] - item_off[b0 + b];
      tiles += fpc_tiles(n, kFpcTileItems);
      capacity += fpc_compressed_bound(n);
    }
  }
  capacity = (capacity + 3) / 4 * 4 + 4;
  hipStream_t stream = library_stream();
  DeviceBuffer<uint32_t> d_items, d_off, d_tile_base, d_tile_sym, d_tile_exc, d_fp_sym, d_fp_exc, d_blob_off;
  DeviceBuffer<uint8_t> d_out;
  Status s;
  if (!(s = d_items.reserve(std::max<uint64_t>(total_items, 1))).ok() || !(s = upload(&d_off, off, stream)).ok() ||
      !(s = upload(&d_tile_base, tile_base, stream)).ok() || !(s = d_tile_sym.reserve(tiles)).ok() || !(s = d_tile_exc.reserve(tiles)).ok() ||
      !(s = d_fp_sym.reserve(count)).ok() || !(s = d_fp_exc.reserve(count)).ok() || !(s = d_blob_off.reserve(count + 1)).ok() ||
      !(s = d_out.reserve(capacity)).ok())
    return s;
  if (total_items)
    NEEDLE_HIP_TRY(hipMemcpyAsync(d_items.ptr, items + item_off[b0], total_items * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  FpcBatch q{};
  q.items = d_items.ptr;
  q.item_off = d_off.ptr;
  q.tile_base = d_tile_base.ptr;
  q.count = count;
  q.tiles = (uint32_t)tiles;
  q.tile_sym = d_tile_sym.ptr;
  q.tile_exc = d_tile_exc.ptr;
  q.fp_sym = d_fp_sym.ptr;
  q.fp_exc = d_fp_exc.ptr;
  q.blob_off = d_blob_off.ptr;
  q.out = d_out.ptr;
  q.out_capacity = (uint32_t)capacity;
  q.algorithm = (uint32_t)algorithm & 0xFF;
  {
    KernelTimer timer("fp_compress_count");
    hipLaunchKernelGGL(fp_compress_count_kernel, dim3(grid_for(tiles)), dim3(kFpcThreads), 0, stream, q);
  }
  {
    KernelTimer timer("fp_compress_layout");
    hipLaunchKernelGGL(fp_compress_layout_kernel, dim3(1), dim3(kFpcThreads), 0, stream, q);
  }
  {
    KernelTimer timer("fp_compress_zero");
    hipLaunchKernelGGL(fp_compress_zero_kernel, dim3(grid_for(capacity / 4 / kFpcThreads + 1)), dim3(kFpcThreads), 0, stream, q);
  }
  {
    KernelTimer timer("fp_compress_pack");
    hipLaunchKernelGGL(fp_compress_pack_kernel, dim3(grid_for(tiles)), dim3(kFpcThreads), 0, stream, q);
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  // only now, behind the last pass: the offsets row, then the bytes it says there are
  std::vector<uint32_t> got(count + 1);
  NEEDLE_HIP_TRY(hipMemcpyAsync(got.data(), d_blob_off.ptr, got.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  const uint64_t total = got[count];
  if (total + 4 > capacity) return Status::Make(NeedleError_Unknown, "fingerprint codec: the layout exceeds the bound");
  const size_t at = blobs->size();
  blobs->resize(at + total);
  if (total) NEEDLE_HIP_TRY(hipMemcpy(blobs->data() + at, d_out.ptr, total, hipMemcpyDeviceToHost));
  for (uint32_t b = 0; b < count; b++) blob_off->push_back(at + got[b + 1]);
  return Status::Ok();
}

Status decompress_batch(const uint8_t *blobs, const uint64_t *blob_off, size_t b0, size_t b1, std::vector<uint32_t> *items,
                        std::vector<uint64_t> *item_off, std::vector<int32_t> *algorithms, std::vector<int32_t> *status) {
  const uint32_t count = (uint32_t)(b1 - b0);
  const uint64_t total_bytes = blob_off[b1] - blob_off[b0];
  const uint8_t *bytes = blobs + blob_off[b0];
  std::vector<uint32_t> off(count + 1), tile_base(count + 1), items_n(count), slot_off(count + 1);
  std::vector<int32_t> verdict(count);
  uint64_t tiles = 0, slots = 0;
  for (uint32_t b = 0; b <= count; b++) {
    off[b] = (uint32_t)(blob_off[b0 + b] - blob_off[b0]);
    tile_base[b] = (uint32_t)tiles;
    slot_off[b] = (uint32_t)slots;
    if (b < count) {
      const uint64_t len = blob_off[b0 + b + 1] - blob_off[b0 + b];
      verdict[b] = fpc_host_verdict(bytes + off[b], len, &items_n[b]);
      algorithms->push_back(len >= 1 ? bytes[off[b]] : 0);
      tiles += fpc_tiles(fpc_max_symbols(len), kFpdTileSymbols);
      slots += items_n[b];
    }
  }
  hipStream_t stream = library_stream();
  DeviceBuffer<uint8_t> d_blobs;
  DeviceBuffer<uint32_t> d_off, d_tile_base, d_items_n, d_slot_off, d_tile_zero, d_tile_seven, d_fp_sym, d_fp_exc, d_bad, d_out;
  DeviceBuffer<int32_t> d_status;
  Status s;
  if (!(s = d_blobs.reserve(std::max<uint64_t>(total_bytes, 1))).ok() || !(s = upload(&d_off, off, stream)).ok() ||
      !(s = upload(&d_tile_base, tile_base, stream)).ok() || !(s = upload(&d_items_n, items_n, stream)).ok() ||
      !(s = upload(&d_slot_off, slot_off, stream)).ok() || !(s = upload(&d_status, verdict, stream)).ok() ||
      !(s = d_tile_zero.reserve(tiles)).ok() || !(s = d_tile_seven.reserve(tiles)).ok() || !(s = d_fp_sym.reserve(count)).ok() ||
      !(s = d_fp_exc.reserve(count)).ok() || !(s = d_bad.reserve(count)).ok() || !(s = d_out.reserve(std::max<uint64_t>(slots, 1))).ok())
    return s;
  if (total_bytes) NEEDLE_HIP_TRY(hipMemcpyAsync(d_blobs.ptr, bytes, total_bytes, hipMemcpyHostToDevice, stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(d_out.ptr, 0, std::max<uint64_t>(slots, 1) * sizeof(uint32_t), stream));
  NEEDLE_HIP_TRY(hipMemsetAsync(d_bad.ptr, 0, count * sizeof(uint32_t), stream));
  FpdBatch q{};
  q.blobs = d_blobs.ptr;
  q.blob_off = d_off.ptr;
  q.tile_base = d_tile_base.ptr;
  q.items_n = d_items_n.ptr;
  q.slot_off = d_slot_off.ptr;
  q.count = count;
  q.tiles = (uint32_t)tiles;
  q.tile_zero = d_tile_zero.ptr;
  q.tile_seven = d_tile_seven.ptr;
  q.fp_sym = d_fp_sym.ptr;
  q.fp_exc = d_fp_exc.ptr;
  q.status = d_status.ptr;
  q.bad = d_bad.ptr;
  q.out = d_out.ptr;
  {
    KernelTimer timer("fp_decompress_count");
    hipLaunchKernelGGL(fp_decompress_count_kernel, dim3(grid_for(tiles)), dim3(kFpcThreads), 0, stream, q);
  }
  {
    KernelTimer timer("fp_decompress_layout");
    hipLaunchKernelGGL(fp_decompress_layout_kernel, dim3(grid_for(count)), dim3(kFpcThreads), 0, stream, q);
  }
  {
    KernelTimer timer("fp_decompress_unpack");
    hipLaunchKernelGGL(fp_decompress_unpack_kernel, dim3(grid_for(tiles)), dim3(kFpcThreads), 0, stream, q);
  }
  {
    KernelTimer timer("fp_decompress_xor");
    hipLaunchKernelGGL(fp_decompress_xor_kernel, dim3(grid_for(count)), dim3(kFpcThreads), 0, stream, q);
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  std::vector<uint32_t> got(std::max<uint64_t>(slots, 1));
  NEEDLE_HIP_TRY(hipMemcpyAsync(verdict.data(), d_status.ptr, count * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipMemcpyAsync(got.data(), d_out.ptr, got.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  for (uint32_t b = 0; b < count; b++) {  // a refused blob's slot is dropped
    if (verdict[b] == kFpcOk) items->insert(items->end(), got.begin() + slot_off[b], got.begin() + slot_off[b] + items_n[b]);
    item_off->push_back(items->size());
    status->push_back(verdict[b]);
  }
  return Status::Ok();
}

Status check_offsets(const uint64_t *off, size_t count, const char *what) {
  for (size_t b = 0; b < count; b++)
    if (off[b + 1] < off[b]) return Status::Make(NeedleError_InvalidArgument, std::string("fingerprint codec: ") + what + " offsets must not decrease");
  return Status::Ok();
}

}  // namespace

Status gpu_fp_compress_host(const uint32_t *items, const uint64_t *item_off, size_t count, int algorithm, std::vector<uint8_t> *blobs,
                            std::vector<uint64_t> *blob_off) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  blobs->clear();
  blob_off->assign(1, 0);
  Status s = check_offsets(item_off, count, "item");
  if (!s.ok()) return s;
  for (size_t b = 0; b < count; b++)
    if (item_off[b + 1] - item_off[b] >= kFpcItemLimit)
      return Status::Make(NeedleError_InvalidArgument, "fingerprint codec: a fingerprint of 2^24 items or more does not fit the header");
  if (!(s = ensure_device()).ok()) return s;
  for (size_t b0 = 0; b0 < count;) {  // batches of at most kFpcBatchItems items and 2^20 fingerprints
    size_t b1 = b0 + 1;
    while (b1 < count && b1 - b0 < (1u << 20) && item_off[b1 + 1] - item_off[b0] <= kFpcBatchItems) b1++;
    if (!(s = compress_batch(items, item_off, b0, b1, algorithm, blobs, blob_off)).ok()) return s;
    b0 = b1;
  }
  return Status::Ok();
}

Status gpu_fp_decompress_host(const uint8_t *blobs, const uint64_t *blob_off, size_t count, std::vector<uint32_t> *items,
                              std::vector<uint64_t> *item_off, std::vector<int32_t> *algorithms, std::vector<int32_t> *status) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  items->clear();
  item_off->assign(1, 0);
  algorithms->clear();
  status->clear();
  Status s = check_offsets(blob_off, count, "blob");
  if (!s.ok()) return s;
  for (size_t b = 0; b < count; b++)
    if (blob_off[b + 1] - blob_off[b] > kFpcBatchBytes)
      return Status::Make(NeedleError_InvalidArgument, "fingerprint codec: a blob of more than 2^30 bytes");
  if (!(s = ensure_device()).ok()) return s;
  for (size_t b0 = 0; b0 < count;) {  // batches of at most kFpcBatchBytes bytes, kFpcBatchItems items and 2^20 blobs
    size_t b1 = b0;
    uint64_t slots = 0;
    while (b1 < count && b1 - b0 < (1u << 20)) {
      const uint64_t len = blob_off[b1 + 1] - blob_off[b1];
      uint32_t n = 0;
      (void)fpc_host_verdict(blobs + blob_off[b1], len, &n);
      if (b1 > b0 && (blob_off[b1 + 1] - blob_off[b0] > kFpcBatchBytes || slots + n > kFpcBatchItems)) break;
      slots += n;
      b1++;
    }
    if (!(s = decompress_batch(blobs, blob_off, b0, b1, items, item_off, algorithms, status)).ok()) return s;
    b0 = b1;
  }
  return Status::Ok();
}

// ---- base64, URL-safe, unpadded (pure host) ------------------------------------------------------------------------
static const char kBase64[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_";

std::string fp_base64_encode(const uint8_t *data, size_t n) {
  std::string out;
  out.reserve((n * 4 + 2) / 3);
  for (size_t i = 0; i < n; i += 3) {
    const size_t have = std::min<size_t>(3, n - i);
    const uint32_t v = ((uint32_t)data[i] << 16) | (have > 1 ? (uint32_t)data[i + 1] << 8 : 0) | (have > 2 ? (uint32_t)data[i + 2] : 0);
    out.push_back(kBase64[(v >> 18) & 63]);
    out.push_back(kBase64[(v >> 12) & 63]);
    if (have > 1) out.push_back(kBase64[(v >> 6) & 63]);
    if (have > 2) out.push_back(kBase64[v & 63]);
  }
  return out;
}

bool fp_base64_decode(const char *text, size_t n, std::vector<uint8_t> *out) {
  out->clear();
  if (n % 4 == 1) return false;
  out->reserve(n * 3 / 4);
  uint32_t acc = 0, bits = 0;
  for (size_t i = 0; i < n; i++) {
    const char c = text[i];
    uint32_t v;
    if (c >= 'A' && c <= 'Z') v = (uint32_t)(c - 'A');
    else if (c >= 'a' && c <= 'z') v = (uint32_t)(c - 'a') + 26;
    else if (c >= '0' && c <= '9') v = (uint32_t)(c - '0') + 52;
    else if (c == '-') v = 62;
    else if (c == '_') v = 63;
    else return false;
    acc = (acc << 6) | v;
    bits += 6;
    if (bits >= 8) {
      bits -= 8;
      out->push_back((uint8_t)(acc >> bits));
      acc &= (1u << bits) - 1;
    }
  }
  return true;  // (left-over bits are dropped, as upstream's decoder drops them)
}

}  // namespace needle
