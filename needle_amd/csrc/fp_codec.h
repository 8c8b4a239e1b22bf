// chromaprint 1.5's fingerprint codec (FingerprintCompressor / FingerprintDecompressor) on the device: fp_codec.hip.
//
// The first half of this file is the codec's INDEX ARITHMETIC: every expression that decides what a lane reads or
// writes -- the symbols of an item, symbol index -> byte and shift, where the two streams of a blob start, the bytes a
// tile covers and which of them it shares with a neighbour, how many items a blob can hold.  They are plain
// __host__ __device__ functions without HIP types, so that tests/cpp/fp_codec_check.cpp runs the same text on the CPU
// (a sequential emulation of the passes over exactly-sized buffers, also under AddressSanitizer) before a kernel ever
// runs.  The second half declares the host drivers.
//
// Format.  x[i] = item[i] ^ item[i-1] (item[-1] = 0).  The set bits of x, from bit 0 up, at 1-based positions p:
// gap = p - last (last = 0, then the previous p); gap < 7: the normal symbol gap; gap >= 7: the normal symbol 7 and the
// exceptional symbol gap - 7 (0..25); behind the last bit the normal symbol 0.  Bytes: [algorithm] [n >> 16] [n >> 8]
// [n], the normal symbols 3 bits each, LSB first, ceil(3 S / 8) bytes, then the exceptional ones 5 bits each,
// ceil(5 E / 8) bytes; padding bits 0.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define FPC_HD __host__ __device__
#else
#define FPC_HD
#endif
#if defined(__clang__)
#define FPC_UNROLL _Pragma("unroll")
#else
#define FPC_UNROLL
#endif

namespace needle {

constexpr uint32_t kFpcThreads = 256;        // lanes of every codec workgroup
constexpr uint32_t kFpcLaneItems = 4;        // consecutive items of a lane
constexpr uint32_t kFpcTileItems = kFpcThreads * kFpcLaneItems;      // compress tile (and the XOR-scan's chunk)
constexpr uint32_t kFpdLaneSymbols = 8;      // consecutive 3-bit symbols of a lane: exactly 3 bytes
constexpr uint32_t kFpdTileSymbols = kFpcThreads * kFpdLaneSymbols;  // decompress tile
constexpr uint32_t kFpcHeaderBytes = 4;
constexpr uint32_t kFpcMaxItemSymbols = 33;  // popcount + 1
constexpr uint32_t kFpcMaxItemExceptional = 4;
constexpr uint64_t kFpcItemLimit = 1ull << 24;  // the header has 24 bits: a fingerprint holds fewer items than this
// one launch chain: items and blob bytes of a batch (32-bit offsets on the device; the drivers cut longer inputs)
constexpr uint64_t kFpcBatchItems = 1ull << 26;
constexpr uint64_t kFpcBatchBytes = 1ull << 30;

enum FpcStatus : int32_t {
  kFpcOk = 0,
  kFpcShortHeader = 1,    // fewer than 4 bytes
  kFpcNormalEnds = 2,     // the 3-bit stream ends before n terminators (or the header claims more than the bytes can hold)
  kFpcExceptionalEnds = 3,
  kFpcBitPosition = 4,    // a bit position above 32
};

// ---- one item ------------------------------------------------------------------------------------------------------
struct FpcItemBits {
  uint64_t lo, hi;  // the normal symbols, 3 bits each, symbol 0 in bits 0..2 of lo (at most 99 bits)
  uint32_t exc;     // the exceptional symbols, 5 bits each (at most 20 bits)
  uint32_t nsym, nexc;
};

FPC_HD inline FpcItemBits fpc_item_bits(uint32_t x) {
  FpcItemBits r{0, 0, 0, 0, 0};
  uint32_t last = 0;
  while (true) {
    uint32_t sym = 0;  // the terminator
    if (x) {
      const uint32_t p = (uint32_t)__builtin_ctz(x) + 1;
      const uint32_t gap = p - last;
      last = p;
      x &= x - 1;
      sym = gap < 7 ? gap : 7;
      if (gap >= 7) {
        r.exc |= (gap - 7) << (5 * r.nexc);
        r.nexc++;
      }
    }
    const uint32_t bit = 3 * r.nsym;
    if (bit < 64) {
      r.lo |= (uint64_t)sym << bit;
      if (bit > 61) r.hi |= (uint64_t)sym >> (64 - bit);
    } else {
      r.hi |= (uint64_t)sym << (bit - 64);
    }
    r.nsym++;
    if (sym == 0) return r;
  }
}

// ---- sizes and stream starts ---------------------------------------------------------------------------------------
FPC_HD inline uint64_t fpc_normal_bytes(uint64_t symbols) { return (3 * symbols + 7) >> 3; }
FPC_HD inline uint64_t fpc_exceptional_bytes(uint64_t exceptional) { return (5 * exceptional + 7) >> 3; }
FPC_HD inline uint64_t fpc_normal_start() { return kFpcHeaderBytes; }                                    // byte of the blob
FPC_HD inline uint64_t fpc_exceptional_start(uint64_t symbols) { return kFpcHeaderBytes + fpc_normal_bytes(symbols); }
FPC_HD inline uint64_t fpc_blob_bytes(uint64_t symbols, uint64_t exceptional) {
  return fpc_exceptional_start(symbols) + fpc_exceptional_bytes(exceptional);
}
// the most a fingerprint of n items can take: 33 normal and 4 exceptional symbols per item
FPC_HD inline uint64_t fpc_compressed_bound(uint64_t n) {
  return fpc_blob_bytes((uint64_t)kFpcMaxItemSymbols * n, (uint64_t)kFpcMaxItemExceptional * n);
}
// the most terminators (items) a blob of `bytes` bytes can hold: whole 3-bit symbols behind the header
FPC_HD inline uint64_t fpc_max_symbols(uint64_t bytes) { return bytes < kFpcHeaderBytes ? 0 : 8 * (bytes - kFpcHeaderBytes) / 3; }
FPC_HD inline uint32_t fpc_header_items(const uint8_t *blob) {
  return ((uint32_t)blob[1] << 16) | ((uint32_t)blob[2] << 8) | (uint32_t)blob[3];
}
// what the host decides from a blob's length and header before anything is allocated: the status (0, 1 or 2) and the
// slot, n items only where the bytes could hold n terminators
FPC_HD inline int32_t fpc_host_verdict(const uint8_t *blob, uint64_t bytes, uint32_t *slot_items) {
  *slot_items = 0;
  if (bytes < kFpcHeaderBytes) return kFpcShortHeader;
  const uint32_t n = fpc_header_items(blob);
  if ((uint64_t)n > fpc_max_symbols(bytes)) return kFpcNormalEnds;
  *slot_items = n;
  return kFpcOk;
}

// ---- tiles ---------------------------------------------------------------------------------------------------------
// Tiles never span two fingerprints: fingerprint b owns fpc_tiles(units_b) of them, at least one (the one that writes the
// header of an empty fingerprint; a blob without symbols has a tile that finds nothing to do).
FPC_HD inline uint64_t fpc_tiles(uint64_t units, uint32_t tile) { return units ? (units + tile - 1) / tile : 1; }

// the last b in [0, count) with base[b] <= t, for t < base[count] (base: count + 1 ascending tile bases, base[0] = 0)
FPC_HD inline uint32_t fpc_tile_owner(const uint32_t *base, uint32_t count, uint32_t t) {
  uint32_t lo = 0, hi = count - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (base[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The bytes of a stream that `units` symbols of `width` bits cover, from symbol `first` of the stream on: bytes
// [first_byte, first_byte + nbytes) of the STREAM (add its start), the first symbol `lead_bits` into the first of them.
struct FpcSpan {
  uint64_t first_byte;
  uint32_t nbytes, lead_bits;
};
FPC_HD inline FpcSpan fpc_tile_span(uint64_t first, uint32_t units, uint32_t width) {
  const uint64_t b0 = first * width, b1 = b0 + (uint64_t)units * width;
  FpcSpan s;
  s.first_byte = b0 >> 3;
  s.lead_bits = (uint32_t)(b0 & 7);
  s.nbytes = units ? (uint32_t)(((b1 + 7) >> 3) - s.first_byte) : 0;
  return s;
}
// The one rule for bytes that two tiles share, or that share an aligned 32-bit word of the output with another tile's,
// another stream's or the header's bytes: the output is zeroed first, and a tile STORES only the aligned words that lie
// wholly inside its span [begin, end) (offsets into the output) without holding the span's first or last byte -- the
// only bytes a neighbour's span can reach.  Every other byte goes in by an atomic OR on the aligned word around it.  So
// no word is both stored and ORed, whatever the order the tiles run in.
FPC_HD inline bool fpc_word_is_owned(uint64_t word, uint64_t begin, uint64_t end) { return word > begin && word + 4 < end; }

// 32-bit words a tile's assembly buffer needs for `units` symbols of `width` bits: up to 7 lead bits, the symbols, and
// the word a shifted value's last piece may fall into
FPC_HD constexpr uint32_t fpc_assembly_words(uint32_t units, uint32_t width) { return (7 + units * width + 31) / 32 + 1; }
constexpr uint32_t kFpcNormalWords = fpc_assembly_words(kFpcTileItems * kFpcMaxItemSymbols, 3);
constexpr uint32_t kFpcExceptionalWords = fpc_assembly_words(kFpcTileItems * kFpcMaxItemExceptional, 5);

// ORs the value hi:lo (at most 99 bits) in at bit `rel` of an assembly buffer of `nwords` words: or_word(word, bits) for
// every word that gets a set bit.  A word beyond the buffer is not touched (and the check fails it: *clipped).
template <class OrWord>
FPC_HD inline void fpc_place_bits(uint32_t rel, uint64_t lo, uint64_t hi, uint32_t nwords, OrWord &&or_word, bool *clipped = nullptr) {
  const uint32_t w0 = rel >> 5, sh = rel & 31;
  const uint32_t v[5] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32), 0};
  uint32_t prev = 0;
  FPC_UNROLL
  for (uint32_t k = 0; k < 5; k++) {
    const uint32_t out = (v[k] << sh) | (sh ? prev >> (32 - sh) : 0);
    prev = v[k];
    if (!out) continue;
    if (w0 + k < nwords) or_word(w0 + k, out);
    else if (clipped) *clipped = true;
  }
}

// ---- reading a blob ------------------------------------------------------------------------------------------------
// `width` (<= 8) bits at bit `bit` of the stream that starts at byte `start` of a blob of `bytes` bytes.  Nothing
// outside [0, bytes) is read: bits from beyond the end are 0.
FPC_HD inline uint32_t fpc_read_bits(const uint8_t *blob, uint64_t bytes, uint64_t start, uint64_t bit, uint32_t width) {
  const uint64_t at = start + (bit >> 3);
  const uint32_t sh = (uint32_t)(bit & 7);
  uint32_t v = at < bytes ? blob[at] : 0;
  if (sh + width > 8 && at + 1 < bytes) v |= (uint32_t)blob[at + 1] << 8;
  return (v >> sh) & ((1u << width) - 1);
}
FPC_HD inline uint32_t fpc_read_symbol(const uint8_t *blob, uint64_t bytes, uint64_t j) {
  return fpc_read_bits(blob, bytes, fpc_normal_start(), 3 * j, 3);
}
// the 8 symbols from symbol j0 (a multiple of 8) on: 3 bytes, symbol i in bits 3i..3i+2
FPC_HD inline uint32_t fpd_lane_load(const uint8_t *blob, uint64_t bytes, uint64_t j0) {
  const uint64_t at = fpc_normal_start() + (j0 >> 3) * 3;
  uint32_t v = 0;
  for (uint32_t k = 0; k < 3; k++)
    if (at + k < bytes) v |= (uint32_t)blob[at + k] << (8 * k);
  return v;
}
// the gap a symbol stands for; `e` is the exceptional index of a seven
FPC_HD inline uint32_t fpd_gap(const uint8_t *blob, uint64_t bytes, uint64_t exc_start, uint32_t sym, uint64_t e) {
  return sym < 7 ? sym : 7 + fpc_read_bits(blob, bytes, exc_start, 5 * e, 5);
}
// The bit position a tile starts at: the gaps of the symbols between the last terminator before symbol `first` and
// `first`, found by walking back.  `sevens_before`: sevens among symbols [0, first).  An item of a well-formed blob has at
// most 33 symbols, so 33 steps without a terminator already sum to more than 32, which the caller refuses.
FPC_HD inline uint32_t fpd_tile_carry(const uint8_t *blob, uint64_t bytes, uint64_t exc_start, uint64_t first, uint64_t sevens_before) {
  uint32_t sum = 0;
  for (uint32_t k = 0; k < kFpcMaxItemSymbols && k < first; k++) {
    const uint32_t sym = fpc_read_symbol(blob, bytes, first - 1 - k);
    if (sym == 0) break;
    if (sym == 7 && sevens_before) sevens_before--;
    sum += fpd_gap(blob, bytes, exc_start, sym, sevens_before);
  }
  return sum;
}

// ---- what one lane of a workgroup does (lane = threadIdx.x; the check calls these for lanes 0..255 in turn) ----------
// compress: the lane's 4 deltas of tile `tile_in_fp` of a fingerprint of n items at `fp` (0 beyond its end), and how many exist
FPC_HD inline uint32_t fpc_lane_deltas(const uint32_t *fp, uint32_t n, uint32_t tile_in_fp, uint32_t lane, uint32_t x[kFpcLaneItems]) {
  const uint64_t i0 = (uint64_t)tile_in_fp * kFpcTileItems + lane * kFpcLaneItems;
  uint32_t have = 0;
  uint32_t prev = (i0 > 0 && i0 <= n) ? fp[i0 - 1] : 0;
  FPC_UNROLL
  for (uint32_t k = 0; k < kFpcLaneItems; k++) {
    x[k] = 0;
    if (i0 + k < n) {
      const uint32_t cur = fp[i0 + k];
      x[k] = cur ^ prev;
      prev = cur;
      have++;
    }
  }
  return have;
}

// compress: bytes [0, span.nbytes) of a tile's assembly buffer go to the stream that starts at byte `stream_at` of the
// output, inside [stream_at, limit).  A lane per aligned word of the output: store(word, value) where the tile owns the
// word, or_word(word, value) otherwise (fpc_word_is_owned).
template <class Store, class OrWord>
FPC_HD inline void fpc_store_span_lane(const uint8_t *assembly, const FpcSpan &span, uint64_t stream_at, uint64_t limit, uint32_t lane,
                                       Store &&store, OrWord &&or_word) {
  const uint64_t begin = stream_at + span.first_byte;
  const uint64_t end = begin + span.nbytes < limit ? begin + span.nbytes : limit;
  for (uint64_t word = (begin & ~(uint64_t)3) + 4 * (uint64_t)lane; word < end; word += 4 * (uint64_t)kFpcThreads) {
    const uint64_t lo = word > begin ? word : begin, hi = word + 4 < end ? word + 4 : end;
    uint32_t value = 0;
    for (uint64_t at = lo; at < hi; at++) value |= (uint32_t)assembly[at - begin] << (8 * (at - word));
    if (fpc_word_is_owned(word, begin, end)) store(word, value);
    else if (value) or_word(word, value);
  }
}

// decompress: the lane's 8 symbols of the tile that starts at symbol `first` (3 bytes), how many of them lie below
// `limit` symbols, and the zeros and sevens among those
FPC_HD inline uint32_t fpd_lane_symbols(const uint8_t *blob, uint64_t bytes, uint64_t first, uint64_t limit, uint32_t lane, uint32_t *valid,
                                        uint32_t *zeros, uint32_t *sevens) {
  const uint64_t j0 = first + (uint64_t)lane * kFpdLaneSymbols;
  const uint32_t v = j0 < limit ? fpd_lane_load(blob, bytes, j0) : 0;
  *valid = j0 >= limit ? 0 : (limit - j0 < kFpdLaneSymbols ? (uint32_t)(limit - j0) : kFpdLaneSymbols);
  uint32_t z = 0, s = 0;
  for (uint32_t i = 0; i < *valid; i++) {
    const uint32_t sym = (v >> (3 * i)) & 7;
    z += sym == 0;
    s += sym == 7;
  }
  *zeros = z;
  *sevens = s;
  return v;
}
// decompress, layout: is the `want`-th zero of the tile among the lane's symbols, `zeros` and `sevens` of the tile lying
// before the lane?  Then *symbols = symbols of the tile up to and with it, *exceptional = sevens of the tile before it.
FPC_HD inline bool fpd_lane_locate(uint32_t v, uint32_t valid, uint32_t lane, uint32_t zeros, uint32_t sevens, uint32_t want,
                                   uint32_t *symbols, uint32_t *exceptional) {
  for (uint32_t i = 0; i < valid; i++) {
    const uint32_t sym = (v >> (3 * i)) & 7;
    if (sym == 0 && ++zeros == want) {
      *symbols = lane * kFpdLaneSymbols + i + 1;
      *exceptional = sevens;
      return true;
    }
    sevens += sym == 7;
  }
  return false;
}
// the segmented sum of gaps: bit 31 = "a terminator lies in the range", bits 0..30 = the gaps behind the range's last terminator
FPC_HD inline uint32_t fpd_seg_combine(uint32_t earlier, uint32_t later) {
  return (later >> 31) ? later : ((earlier & 0x80000000u) | ((earlier + later) & 0x7FFFFFFFu));
}
// decompress, unpack: the gaps of the lane's symbols (0 = terminator; e = exceptional index of the lane's first seven),
// and the lane's share of the segmented sum
FPC_HD inline uint32_t fpd_lane_gaps(const uint8_t *blob, uint64_t bytes, uint64_t exc_start, uint32_t v, uint32_t valid, uint64_t e,
                                     uint32_t gap[kFpdLaneSymbols]) {
  uint32_t seg = 0;
  FPC_UNROLL
  for (uint32_t i = 0; i < kFpdLaneSymbols; i++) {
    gap[i] = 0;
    if (i < valid) {
      const uint32_t sym = (v >> (3 * i)) & 7;
      gap[i] = fpd_gap(blob, bytes, exc_start, sym, e);
      e += sym == 7;
      seg = fpd_seg_combine(seg, sym == 0 ? 0x80000000u : gap[i]);
    }
  }
  return seg;
}
// decompress, unpack: the lane's bits -> or_item(item, bits) for items below n; `item`: the item of the lane's first
// symbol, `pos`: the bit position reached before it.  False if a position exceeds 32.
template <class OrItem>
FPC_HD inline bool fpd_lane_emit(const uint32_t gap[kFpdLaneSymbols], uint32_t valid, uint32_t item, uint32_t pos, uint32_t n, OrItem &&or_item) {
  uint32_t acc = 0;
  bool good = true;
  FPC_UNROLL
  for (uint32_t i = 0; i < kFpdLaneSymbols; i++) {
    if (i >= valid) continue;
    if (gap[i] == 0) {  // a terminator: the item is complete
      if (acc && item < n) or_item(item, acc);
      item++;
      pos = 0;
      acc = 0;
    } else {
      pos += gap[i];
      if (pos > 32) good = false;
      else acc |= 1u << (pos - 1);
    }
  }
  if (acc && item < n) or_item(item, acc);
  return good;
}

// ---- host drivers (fp_codec.hip) -----------------------------------------------------------------------------------
#if !defined(FP_CODEC_ARITHMETIC_ONLY)
}  // namespace needle
#include <vector>

#include "common.h"
namespace needle {
// Fingerprints item_off[b] .. item_off[b + 1] of `items` (host) -> their blobs, concatenated, blob b at blob_off[b].
// InvalidArgument, with nothing done, for offsets that are not monotone or a fingerprint of 2^24 items or more.
Status gpu_fp_compress_host(const uint32_t *items, const uint64_t *item_off, size_t count, int algorithm,
                            std::vector<uint8_t> *blobs, std::vector<uint64_t> *blob_off);
// Blobs blob_off[b] .. blob_off[b + 1] of `blobs` (host) -> items, algorithm byte and FpcStatus per blob; a refused
// blob has an empty slot.
Status gpu_fp_decompress_host(const uint8_t *blobs, const uint64_t *blob_off, size_t count, std::vector<uint32_t> *items,
                              std::vector<uint64_t> *item_off, std::vector<int32_t> *algorithms, std::vector<int32_t> *status);
// URL-safe base64 without padding; decode refuses characters outside the alphabet and a length of 1 mod 4
std::string fp_base64_encode(const uint8_t *data, size_t n);
bool fp_base64_decode(const char *text, size_t n, std::vector<uint8_t> *out);
#endif

}  // namespace needle
