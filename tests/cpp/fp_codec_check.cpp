// The fingerprint codec's index arithmetic (needle_amd/csrc/fp_codec.h) on the CPU: a sequential emulation of the device
// passes -- tile by tile, lane by lane, through the same functions the kernels call -- over exactly-sized heap buffers,
// held against a plain sequential codec written from the format's description.  Stand-alone: it runs as it is and under
// AddressSanitizer / UndefinedBehaviorSanitizer, so an index out of range is found without a device.
//
//   fp_codec_check                      the checks; prints "fp codec ok"
//   fp_codec_check bench FPS ITEMS      the plain sequential codec alone over FPS fingerprints of ITEMS random-delta items:
//                                       one JSON line with its seconds (the yardstick of tools/bench_fp_codec.py)
#define FP_CODEC_ARITHMETIC_ONLY
#include "fp_codec.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace needle;

static int failures = 0;
#define CHECK(cond, ...)                                       \
  do {                                                         \
    if (!(cond)) {                                             \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                \
      std::printf("\n");                                       \
      if (++failures > 20) std::exit(1);                       \
    }                                                          \
  } while (0)

using Bytes = std::vector<uint8_t>;
using Items = std::vector<uint32_t>;

// ---- the plain sequential codec ------------------------------------------------------------------------------------
struct BitWriter {
  Bytes *out;
  uint32_t acc = 0, bits = 0;
  void put(uint32_t v, uint32_t width) {
    acc |= v << bits;
    bits += width;
    while (bits >= 8) {
      out->push_back((uint8_t)acc);
      acc >>= 8;
      bits -= 8;
    }
  }
  void flush() {
    if (bits) out->push_back((uint8_t)acc);
    acc = bits = 0;
  }
};

static Bytes plain_compress(const uint32_t *items, size_t n, int algorithm) {
  Bytes out = {(uint8_t)algorithm, (uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n};
  Bytes exceptional;
  BitWriter normal{&out}, exc{&exceptional};
  uint32_t prev = 0;
  for (size_t i = 0; i < n; i++) {
    uint32_t x = items[i] ^ prev, last = 0;
    prev = items[i];
    for (; x; x &= x - 1) {
      const uint32_t p = (uint32_t)__builtin_ctz(x) + 1, gap = p - last;
      last = p;
      if (gap < 7) {
        normal.put(gap, 3);
      } else {
        normal.put(7, 3);
        exc.put(gap - 7, 5);
      }
    }
    normal.put(0, 3);
  }
  normal.flush();
  exc.flush();
  out.insert(out.end(), exceptional.begin(), exceptional.end());
  return out;
}

static int plain_decompress(const Bytes &blob, Items *items, int *algorithm) {
  items->clear();
  *algorithm = blob.empty() ? 0 : blob[0];
  if (blob.size() < 4) return 1;
  const size_t n = ((size_t)blob[1] << 16) | ((size_t)blob[2] << 8) | blob[3];
  const size_t available = 8 * (blob.size() - 4) / 3;
  auto bits_at = [&](size_t start, size_t bit, uint32_t width) {
    const size_t at = start + (bit >> 3);
    uint32_t v = at < blob.size() ? blob[at] : 0;
    if (at + 1 < blob.size()) v |= (uint32_t)blob[at + 1] << 8;
    return (v >> (bit & 7)) & ((1u << width) - 1);
  };
  std::vector<uint8_t> normal;
  size_t zeros = 0, sevens = 0;
  while (zeros < n) {
    if (normal.size() >= available) return 2;
    normal.push_back((uint8_t)bits_at(4, 3 * normal.size(), 3));
    zeros += normal.back() == 0;
    sevens += normal.back() == 7;
  }
  const size_t start = 4 + (3 * normal.size() + 7) / 8;
  if (start + (5 * sevens + 7) / 8 > blob.size()) return 3;
  uint32_t x = 0, pos = 0, prev = 0;
  size_t e = 0;
  Items out;
  for (uint8_t s : normal) {
    if (s == 0) {
      prev ^= x;
      out.push_back(prev);
      x = pos = 0;
      continue;
    }
    pos += s == 7 ? 7 + bits_at(start, 5 * e++, 5) : s;
    if (pos > 32) return 4;
    x |= 1u << (pos - 1);
  }
  *items = out;
  return 0;
}

// ---- the emulation of the device passes ----------------------------------------------------------------------------
// what block_scan gives each lane, for values in lane order
template <class Op>
static void scan256(const uint32_t v[kFpcThreads], Op op, uint32_t incl[kFpcThreads], uint32_t excl[kFpcThreads], uint32_t *total) {
  uint32_t run = 0;
  for (uint32_t l = 0; l < kFpcThreads; l++) {
    excl[l] = run;
    run = l ? op(run, v[l]) : op(0u, v[l]);
    incl[l] = run;
  }
  *total = run;
}
static uint32_t add_op(uint32_t a, uint32_t b) { return a + b; }

static std::vector<uint32_t> tile_bases(const std::vector<uint64_t> &units, uint32_t tile) {
  std::vector<uint32_t> base(units.size() + 1, 0);
  for (size_t b = 0; b < units.size(); b++) base[b + 1] = base[b] + (uint32_t)fpc_tiles(units[b], tile);
  return base;
}

static void emul_compress(const Items &all, const std::vector<uint64_t> &off, int algorithm, std::vector<Bytes> *blobs) {
  const uint32_t count = (uint32_t)(off.size() - 1);
  blobs->assign(count, Bytes());
  if (!count) return;
  // every fingerprint in a heap block of exactly its size: a read past its end is an error the sanitizer sees
  std::vector<std::unique_ptr<uint32_t[]>> fp(count);
  std::vector<uint64_t> n(count);
  for (uint32_t b = 0; b < count; b++) {
    n[b] = off[b + 1] - off[b];
    fp[b].reset(new uint32_t[n[b]]);
    if (n[b]) std::memcpy(fp[b].get(), all.data() + off[b], n[b] * sizeof(uint32_t));
  }
  const std::vector<uint32_t> base = tile_bases(n, kFpcTileItems);
  const uint32_t tiles = base[count];
  std::vector<uint32_t> tile_sym(tiles), tile_exc(tiles), fp_sym(count), fp_exc(count);
  // count
  for (uint32_t t = 0; t < tiles; t++) {
    const uint32_t b = fpc_tile_owner(base.data(), count, t);
    CHECK(base[b] <= t && t < base[b + 1], "tile %u owner %u", t, b);
    uint32_t s = 0, e = 0;
    for (uint32_t lane = 0; lane < kFpcThreads; lane++) {
      uint32_t x[kFpcLaneItems];
      const uint32_t have = fpc_lane_deltas(fp[b].get(), (uint32_t)n[b], t - base[b], lane, x);
      for (uint32_t k = 0; k < have; k++) {
        const FpcItemBits bits = fpc_item_bits(x[k]);
        s += bits.nsym;
        e += bits.nexc;
      }
    }
    CHECK(s < 65536 && e < 65536, "a tile's counts fit 16 bits");
    tile_sym[t] = s;
    tile_exc[t] = e;
  }
  // layout
  std::vector<uint64_t> blob_off(count + 1, 0);
  for (uint32_t b = 0; b < count; b++) {
    uint32_t s = 0, e = 0;
    for (uint32_t t = base[b]; t < base[b + 1]; t++) {
      const uint32_t ts = tile_sym[t], te = tile_exc[t];
      tile_sym[t] = s;
      tile_exc[t] = e;
      s += ts;
      e += te;
    }
    fp_sym[b] = s;
    fp_exc[b] = e;
    blob_off[b + 1] = blob_off[b] + fpc_blob_bytes(s, e);
    CHECK(fpc_blob_bytes(s, e) <= fpc_compressed_bound(n[b]), "blob %u exceeds the bound", b);
  }
  // zero: the output, exactly as long as the layout says (the device rounds up to a word; no set bit may land there)
  const uint64_t total = blob_off[count];
  std::unique_ptr<uint8_t[]> out(new uint8_t[total]());
  std::vector<uint8_t> how(total, 0);  // 1: stored, 2: ORed
  // pack
  std::unique_ptr<uint32_t[]> normal(new uint32_t[kFpcNormalWords]), exceptional(new uint32_t[kFpcExceptionalWords]);
  for (uint32_t t = 0; t < tiles; t++) {
    const uint32_t b = fpc_tile_owner(base.data(), count, t), tile_in_fp = t - base[b];
    std::memset(normal.get(), 0, kFpcNormalWords * 4);
    std::memset(exceptional.get(), 0, kFpcExceptionalWords * 4);
    uint32_t packed[kFpcThreads], incl[kFpcThreads], excl[kFpcThreads], tot;
    std::vector<FpcItemBits> bits(kFpcThreads * kFpcLaneItems);
    std::vector<uint32_t> have(kFpcThreads);
    for (uint32_t lane = 0; lane < kFpcThreads; lane++) {
      uint32_t x[kFpcLaneItems];
      have[lane] = fpc_lane_deltas(fp[b].get(), (uint32_t)n[b], tile_in_fp, lane, x);
      packed[lane] = 0;
      for (uint32_t k = 0; k < kFpcLaneItems; k++) {
        bits[lane * kFpcLaneItems + k] = fpc_item_bits(x[k]);
        if (k < have[lane]) packed[lane] += bits[lane * kFpcLaneItems + k].nsym | (bits[lane * kFpcLaneItems + k].nexc << 16);
      }
    }
    scan256(packed, add_op, incl, excl, &tot);
    const FpcSpan ns = fpc_tile_span(tile_sym[t], tot & 0xFFFF, 3), es = fpc_tile_span(tile_exc[t], tot >> 16, 5);
    CHECK(ns.nbytes <= kFpcNormalWords * 4 && es.nbytes <= kFpcExceptionalWords * 4, "a span fits its assembly buffer");
    for (uint32_t lane = 0; lane < kFpcThreads; lane++) {
      uint32_t s = excl[lane] & 0xFFFF, e = excl[lane] >> 16;
      for (uint32_t k = 0; k < have[lane]; k++) {
        const FpcItemBits &ib = bits[lane * kFpcLaneItems + k];
        bool clipped = false;
        fpc_place_bits(ns.lead_bits + 3 * s, ib.lo, ib.hi, kFpcNormalWords, [&](uint32_t w, uint32_t v) { normal[w] |= v; }, &clipped);
        fpc_place_bits(es.lead_bits + 5 * e, ib.exc, 0, kFpcExceptionalWords, [&](uint32_t w, uint32_t v) { exceptional[w] |= v; }, &clipped);
        CHECK(!clipped, "tile %u lane %u: bits beyond the assembly buffer", t, lane);
        s += ib.nsym;
        e += ib.nexc;
      }
    }
    const uint64_t blob_at = blob_off[b], blob_end = blob_off[b + 1];
    auto store = [&](uint64_t word, uint32_t value) {
      for (uint32_t k = 0; k < 4; k++) {
        CHECK(word + k >= blob_at + kFpcHeaderBytes && word + k < blob_end, "tile %u stores outside its blob", t);
        if (word + k >= total) return;
        CHECK(how[word + k] == 0, "byte %llu stored and written before", (unsigned long long)(word + k));
        how[word + k] = 1;
        out[word + k] = (uint8_t)(value >> (8 * k));
      }
    };
    auto or_word = [&](uint64_t word, uint32_t value) {
      for (uint32_t k = 0; k < 4; k++) {
        const uint8_t v = (uint8_t)(value >> (8 * k));
        if (!v) continue;
        CHECK(word + k >= blob_at && word + k < blob_end, "tile %u ORs outside its blob", t);
        if (word + k >= total) return;
        CHECK(how[word + k] != 1, "byte %llu ORed and stored", (unsigned long long)(word + k));
        how[word + k] = 2;
        out[word + k] |= v;
      }
    };
    for (uint32_t lane = 0; lane < kFpcThreads; lane++) {
      fpc_store_span_lane(reinterpret_cast<const uint8_t *>(normal.get()), ns, blob_at + fpc_normal_start(), blob_end, lane, store, or_word);
      fpc_store_span_lane(reinterpret_cast<const uint8_t *>(exceptional.get()), es, blob_at + fpc_exceptional_start(fp_sym[b]), blob_end, lane,
                          store, or_word);
    }
    if (tile_in_fp == 0) {
      const uint32_t hdr[4] = {(uint32_t)algorithm & 0xFF, (uint32_t)(n[b] >> 16) & 0xFF, (uint32_t)(n[b] >> 8) & 0xFF, (uint32_t)n[b] & 0xFF};
      for (uint32_t k = 0; k < 4; k++) {
        const uint64_t at = blob_at + k;
        or_word(at & ~(uint64_t)3, hdr[k] << (8 * (at & 3)));
      }
    }
  }
  for (uint32_t b = 0; b < count; b++) (*blobs)[b].assign(out.get() + blob_off[b], out.get() + blob_off[b + 1]);
}

struct Decoded {
  std::vector<Items> items;
  std::vector<int32_t> algorithm, status;
};

static Decoded emul_decompress(const std::vector<Bytes> &blobs) {
  const uint32_t count = (uint32_t)blobs.size();
  Decoded d;
  d.items.assign(count, Items());
  d.algorithm.assign(count, 0);
  d.status.assign(count, 0);
  if (!count) return d;
  std::vector<std::unique_ptr<uint8_t[]>> blob(count);  // exactly-sized copies
  std::vector<uint64_t> len(count), symbols(count);
  std::vector<uint32_t> items_n(count);
  std::vector<std::unique_ptr<uint32_t[]>> slot(count);
  for (uint32_t b = 0; b < count; b++) {
    len[b] = blobs[b].size();
    blob[b].reset(new uint8_t[len[b]]);
    if (len[b]) std::memcpy(blob[b].get(), blobs[b].data(), len[b]);
    d.status[b] = fpc_host_verdict(blob[b].get(), len[b], &items_n[b]);
    d.algorithm[b] = len[b] ? blob[b][0] : 0;
    symbols[b] = fpc_max_symbols(len[b]);
    slot[b].reset(new uint32_t[items_n[b]]());
  }
  const std::vector<uint32_t> base = tile_bases(symbols, kFpdTileSymbols);
  const uint32_t tiles = base[count];
  std::vector<uint32_t> tile_zero(tiles, 0), tile_seven(tiles, 0), fp_sym(count, 0), fp_exc(count, 0);
  // count
  for (uint32_t t = 0; t < tiles; t++) {
    const uint32_t b = fpc_tile_owner(base.data(), count, t);
    CHECK(base[b] <= t && t < base[b + 1], "tile %u owner %u", t, b);
    if (d.status[b] != kFpcOk) continue;
    for (uint32_t lane = 0; lane < kFpcThreads; lane++) {
      uint32_t valid, z, s;
      fpd_lane_symbols(blob[b].get(), len[b], (uint64_t)(t - base[b]) * kFpdTileSymbols, symbols[b], lane, &valid, &z, &s);
      tile_zero[t] += z;
      tile_seven[t] += s;
    }
  }
  // layout
  for (uint32_t b = 0; b < count; b++) {
    const uint32_t n = items_n[b];
    if (d.status[b] != kFpcOk || n == 0) continue;
    uint32_t zeros_before = 0, sevens_before = 0, found_t = 0, found_z = 0, found_s = 0;
    bool found = false;
    for (uint32_t cb = base[b]; cb < base[b + 1] && !found; cb += kFpcThreads) {
      uint32_t z[kFpcThreads], s[kFpcThreads], zi[kFpcThreads], ze[kFpcThreads], si[kFpcThreads], se[kFpcThreads], zt, st;
      for (uint32_t lane = 0; lane < kFpcThreads; lane++) {
        const uint32_t t = cb + lane;
        z[lane] = t < base[b + 1] ? tile_zero[t] : 0;
        s[lane] = t < base[b + 1] ? tile_seven[t] : 0;
      }
      scan256(z, add_op, zi, ze, &zt);
      scan256(s, add_op, si, se, &st);
      for (uint32_t lane = 0; lane < kFpcThreads; lane++) {
        const uint32_t t = cb + lane;
        if (t >= base[b + 1]) continue;
        tile_zero[t] = zeros_before + ze[lane];
        tile_seven[t] = sevens_before + se[lane];
        if (zeros_before + ze[lane] < n && zeros_before + zi[lane] >= n) {
          CHECK(!found, "two tiles claim the n-th zero");
          found = true;
          found_t = t;
          found_z = zeros_before + ze[lane];
          found_s = sevens_before + se[lane];
        }
      }
      zeros_before += zt;
      sevens_before += st;
    }
    if (!found) {
      d.status[b] = kFpcNormalEnds;
      continue;
    }
    const uint64_t first = (uint64_t)(found_t - base[b]) * kFpdTileSymbols;
    uint32_t packed[kFpcThreads], v[kFpcThreads], valid[kFpcThreads], incl[kFpcThreads], excl[kFpcThreads], tot;
    for (uint32_t lane = 0; lane < kFpcThreads; lane++) {
      uint32_t z, s;
      v[lane] = fpd_lane_symbols(blob[b].get(), len[b], first, symbols[b], lane, &valid[lane], &z, &s);
      packed[lane] = z | (s << 16);
    }
    scan256(packed, add_op, incl, excl, &tot);
    uint32_t hits = 0;
    for (uint32_t lane = 0; lane < kFpcThreads; lane++) {
      uint32_t in_tile, sevens_in_tile;
      if (!fpd_lane_locate(v[lane], valid[lane], lane, excl[lane] & 0xFFFF, excl[lane] >> 16, n - found_z, &in_tile, &sevens_in_tile)) continue;
      hits++;
      const uint64_t S = first + in_tile, E = (uint64_t)found_s + sevens_in_tile;
      fp_sym[b] = (uint32_t)S;
      fp_exc[b] = (uint32_t)E;
      if (fpc_blob_bytes(S, E) > len[b]) d.status[b] = kFpcExceptionalEnds;
    }
    CHECK(hits == 1, "blob %u: %u lanes found the n-th zero", b, hits);
  }
  // unpack
  for (uint32_t t = 0; t < tiles; t++) {
    const uint32_t b = fpc_tile_owner(base.data(), count, t);
    const uint64_t S = fp_sym[b], first = (uint64_t)(t - base[b]) * kFpdTileSymbols;
    if (d.status[b] != kFpcOk || first >= S) continue;
    const uint64_t exc_start = fpc_exceptional_start(S);
    const uint32_t n = items_n[b];
    const uint32_t carry = fpd_tile_carry(blob[b].get(), len[b], exc_start, first, tile_seven[t]);
    uint32_t packed[kFpcThreads], v[kFpcThreads], valid[kFpcThreads], incl[kFpcThreads], counts[kFpcThreads], tot;
    for (uint32_t lane = 0; lane < kFpcThreads; lane++) {
      uint32_t z, s;
      v[lane] = fpd_lane_symbols(blob[b].get(), len[b], first, S, lane, &valid[lane], &z, &s);
      packed[lane] = z | (s << 16);
    }
    scan256(packed, add_op, incl, counts, &tot);
    uint32_t seg[kFpcThreads], seg_incl[kFpcThreads], before[kFpcThreads], seg_tot;
    std::vector<uint32_t> gaps(kFpcThreads * kFpdLaneSymbols);
    for (uint32_t lane = 0; lane < kFpcThreads; lane++)
      seg[lane] = fpd_lane_gaps(blob[b].get(), len[b], exc_start, v[lane], valid[lane], (uint64_t)tile_seven[t] + (counts[lane] >> 16),
                                &gaps[lane * kFpdLaneSymbols]);
    scan256(seg, fpd_seg_combine, seg_incl, before, &seg_tot);
    for (uint32_t lane = 0; lane < kFpcThreads; lane++) {
      const uint32_t pos = (before[lane] & 0x7FFFFFFFu) + ((before[lane] >> 31) ? 0 : carry);
      const bool good = fpd_lane_emit(&gaps[lane * kFpdLaneSymbols], valid[lane], tile_zero[t] + (counts[lane] & 0xFFFF), pos, n,
                                      [&](uint32_t item, uint32_t bits) {
                                        CHECK(item < n, "blob %u: item %u outside its slot of %u", b, item, n);
                                        CHECK((slot[b][item] & bits) == 0, "blob %u item %u: a bit set twice", b, item);
                                        slot[b][item] |= bits;
                                      });
      if (!good) d.status[b] = kFpcBitPosition;
    }
  }
  // xor
  for (uint32_t b = 0; b < count; b++) {
    if (d.status[b] != kFpcOk) continue;
    const uint32_t n = items_n[b];
    uint32_t carry = 0;
    for (uint32_t cb = 0; cb < n; cb += kFpcTileItems) {
      uint32_t chunk = 0;
      for (uint32_t lane = 0; lane < kFpcThreads; lane++) {
        uint32_t run = carry ^ chunk;
        for (uint32_t k = 0; k < kFpcLaneItems; k++) {
          const uint32_t i = cb + lane * kFpcLaneItems + k;
          if (i >= n) continue;
          run ^= slot[b][i];
          chunk ^= slot[b][i];
          slot[b][i] = run;
        }
      }
      carry ^= chunk;
    }
    d.items[b].assign(slot[b].get(), slot[b].get() + n);
  }
  return d;
}

// ---- the checks ----------------------------------------------------------------------------------------------------
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

static Items make_items(size_t n, int kind) {
  Items it(n);
  uint32_t prev = 0;
  for (size_t i = 0; i < n; i++) {
    uint32_t x = 0;
    switch (kind) {
      case 0: x = 0; break;                                        // terminators only
      case 1: x = 0xFFFFFFFFu; break;                              // items alternate 0xFFFFFFFF, 0: 33 symbols each
      case 2: x = 1u << 31; break;                                 // gap 32
      case 3: x = (i & 1) ? 0x41u : 0x81u; break;                  // gap 6 against gap 7
      case 4: x = 0x80000001u; break;                              // bits 0 and 31
      case 5: x = (1u << 6) | (1u << 13) | (1u << 20) | (1u << 27); break;  // four gaps of 7: the most exceptional symbols
      default: {
        const uint32_t bits = rnd() % 9;
        for (uint32_t k = 0; k < bits; k++) x |= 1u << (rnd() & 31);
      }
    }
    prev ^= x;
    it[i] = prev;
  }
  return it;
}

static Bytes from_base64(const char *text) {
  static const char alphabet[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_";
  Bytes out;
  uint32_t acc = 0, bits = 0;
  for (; *text; text++) {
    acc = (acc << 6) | (uint32_t)(std::strchr(alphabet, *text) - alphabet);
    bits += 6;
    if (bits >= 8) {
      bits -= 8;
      out.push_back((uint8_t)(acc >> bits));
    }
  }
  return out;
}

// the emulation against the plain codec for a batch of blobs: statuses, items, algorithms
static void check_decode(const std::vector<Bytes> &blobs, const char *what) {
  const Decoded d = emul_decompress(blobs);
  for (size_t b = 0; b < blobs.size(); b++) {
    Items want;
    int algorithm = 0;
    const int status = plain_decompress(blobs[b], &want, &algorithm);
    CHECK(d.status[b] == status, "%s blob %zu (%zu bytes): status %d, the plain codec says %d", what, b, blobs[b].size(), d.status[b], status);
    CHECK(d.algorithm[b] == algorithm, "%s blob %zu: algorithm", what, b);
    CHECK(d.items[b] == want, "%s blob %zu: items differ", what, b);
  }
}

static void check_batch(const std::vector<Items> &fps, int algorithm, const char *what) {
  Items all;
  std::vector<uint64_t> off = {0};
  for (const Items &f : fps) {
    all.insert(all.end(), f.begin(), f.end());
    off.push_back(all.size());
  }
  std::vector<Bytes> blobs;
  emul_compress(all, off, algorithm, &blobs);
  for (size_t b = 0; b < fps.size(); b++) {
    const Bytes want = plain_compress(fps[b].data(), fps[b].size(), algorithm);
    CHECK(blobs[b] == want, "%s fingerprint %zu (%zu items): bytes differ from the plain codec's", what, b, fps[b].size());
    blobs[b] = want;
  }
  const Decoded d = emul_decompress(blobs);
  for (size_t b = 0; b < fps.size(); b++) {
    CHECK(d.status[b] == 0 && d.algorithm[b] == (algorithm & 0xFF), "%s fingerprint %zu: status %d", what, b, d.status[b]);
    CHECK(d.items[b] == fps[b], "%s fingerprint %zu: round trip", what, b);
  }
}

static int run_checks() {
  struct Vector {
    Items items;
    int algorithm;
    Bytes bytes;
  };
  const std::vector<Vector> vectors = {
      {{}, 0, {0, 0, 0, 0}},
      {{1}, 0, {0, 0, 0, 1, 1}},
      {{7}, 0, {0, 0, 0, 1, 73, 0}},
      {{1u << 6}, 0, {0, 0, 0, 1, 7, 0}},
      {{1u << 8}, 0, {0, 0, 0, 1, 7, 2}},
      {{1, 0}, 0, {0, 0, 0, 2, 65, 0}},
      {{1, 1}, 0, {0, 0, 0, 2, 1, 0}},
      {{1u << 31}, 0, {0, 0, 0, 1, 7, 25}},
      {{0x80000001u}, 0, {0, 0, 0, 1, 57, 0, 24}},
      {{627964279u, 627964279u, 627964279u}, 1, from_base64("AQAAA0mUaEkSRZEGAA")},
  };
  // the ten vectors: the plain codec, the emulation one by one and as one batch
  for (size_t k = 0; k < vectors.size(); k++) {
    const Vector &v = vectors[k];
    CHECK(plain_compress(v.items.data(), v.items.size(), v.algorithm) == v.bytes, "vector %zu: plain codec", k);
    std::vector<Bytes> blobs;
    emul_compress(v.items, {0, v.items.size()}, v.algorithm, &blobs);
    CHECK(blobs[0] == v.bytes, "vector %zu: emulation", k);
    const Decoded d = emul_decompress({v.bytes});
    CHECK(d.status[0] == 0 && d.items[0] == v.items && d.algorithm[0] == v.algorithm, "vector %zu: decode", k);
    // every truncation, byte by byte
    std::vector<Bytes> cuts;
    for (size_t len = 0; len <= v.bytes.size(); len++) cuts.push_back(Bytes(v.bytes.begin(), v.bytes.begin() + len));
    check_decode(cuts, "truncation");
  }
  {
    std::vector<Items> fps;
    for (const Vector &v : vectors)
      if (v.algorithm == 0) fps.push_back(v.items);
    check_batch(fps, 0, "vectors");
  }
  // sizes and the bound
  CHECK(fpc_compressed_bound(0) == 4 && fpc_compressed_bound(1) == 4 + 13 + 3 && fpc_compressed_bound(3) == 4 + 38 + 8, "bound");
  for (uint32_t x : {0xFFFFFFFFu, 0x40810204u | 1u, 0u, 0x80000000u}) {
    const FpcItemBits bits = fpc_item_bits(x);
    CHECK(bits.nsym == (uint32_t)__builtin_popcount(x) + 1 && bits.nsym <= kFpcMaxItemSymbols && bits.nexc <= kFpcMaxItemExceptional, "item %08x", x);
  }
  CHECK(fpc_item_bits((1u << 6) | (1u << 13) | (1u << 20) | (1u << 27)).nexc == 4, "four gaps of 7");
  // forged headers, a bit position of 33, trailing garbage, and the [0x80000001, 1 << 8, 7] blob cut everywhere
  {
    std::vector<Bytes> blobs = {
        {0, 0xFF, 0xFF, 0xFF},           // n = 2^24 - 1 on four bytes
        {0, 0, 0, 3, 0},                 // n above floor(8 (L - 4) / 3) = 2
        {0, 0, 0, 2, 0},                 // n at the bound
        {0, 0, 0, 1, 15, 0, 25},         // symbols 7, 1, 0 with exceptional 25: positions 32 and 33
        {0, 0, 0, 1, 0x49, 0x92, 0x24, 0x49, 0x92, 0x24, 0x49, 0x92, 0x24, 0x49, 0x92, 0x24, 0x01, 0},  // 33 ones, then 0: position 33
        {1, 0, 0, 0, 0xAB, 0xCD},        // n = 0 and garbage behind the header
        {},
        {9},
    };
    const uint32_t three[3] = {0x80000001u, 1u << 8, 7};
    const Bytes blob = plain_compress(three, 3, 1);
    for (size_t len = 0; len <= blob.size(); len++) blobs.push_back(Bytes(blob.begin(), blob.begin() + len));
    Bytes garbage = blob;
    for (int k = 0; k < 9; k++) garbage.push_back((uint8_t)(0xF0 + k));
    blobs.push_back(garbage);
    blobs.push_back(blob);
    check_decode(blobs, "refusals");
    const Decoded d = emul_decompress(blobs);
    CHECK(d.status[0] == 2 && d.status[1] == 2 && d.status[2] == 0 && d.status[3] == 4 && d.status[4] == 4 && d.status[5] == 0 && d.status[6] == 1 &&
              d.status[7] == 1,
          "the refusals' statuses");
    CHECK(d.status[blobs.size() - 2] == 0 && d.items[blobs.size() - 2] == Items(three, three + 3), "trailing bytes are ignored");
  }
  // batches around the compress tile: empty fingerprints, ends exactly on a tile edge, every kind of content
  const uint32_t T = kFpcTileItems, D = kFpdTileSymbols;
  for (int kind = 0; kind <= 6; kind++) {
    std::vector<Items> fps;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)T - 1, (size_t)T, (size_t)0, (size_t)T + 1, (size_t)3 * T + 5, (size_t)0})
      fps.push_back(make_items(n, kind));
    check_batch(fps, kind, "tile edges");
  }
  // around the decompress tile: all-zero fingerprints have exactly n symbols; a dense one spans tiles
  {
    std::vector<Items> fps = {make_items(D - 1, 0), make_items(D, 0), make_items(D + 1, 0), make_items(2 * D / 33 + 40, 1), make_items(3 * D, 6)};
    check_batch(fps, 1, "symbol tile edges");
  }
  // damaged blobs: bytes flipped and blobs cut at random, also across tile edges; the emulation and the plain codec agree
  for (int round = 0; round < 40; round++) {
    std::vector<Bytes> blobs;
    for (int k = 0; k < 6; k++) {
      const Items it = make_items(rnd() % 700, k == 0 ? 1 : 6);
      Bytes blob = plain_compress(it.data(), it.size(), 1);
      const uint32_t what = rnd() % 4;
      if (what == 0 && blob.size() > 4) blob.resize(4 + rnd() % (blob.size() - 4));
      if (what == 1)
        for (int f = 0; f < 3; f++) blob[rnd() % blob.size()] ^= (uint8_t)(1u << (rnd() & 7));
      if (what == 2 && blob.size() > 8) {  // a long run of ones without a terminator, wherever it falls
        const size_t at = 4 + rnd() % (blob.size() - 8);
        for (size_t j = at; j < blob.size() && j < at + 16; j++) blob[j] = (uint8_t)(j % 3 == 0 ? 0x49 : j % 3 == 1 ? 0x92 : 0x24);
      }
      blobs.push_back(blob);
    }
    check_decode(blobs, "damaged");
  }
  if (failures) return 1;
  std::printf("fp codec ok\n");
  return 0;
}

static int run_bench(size_t fps, size_t n) {
  std::vector<Items> items(fps);
  for (Items &it : items) it = make_items(n, 6);
  std::vector<Bytes> blobs(fps);
  auto t0 = std::chrono::steady_clock::now();
  size_t bytes = 0;
  for (size_t b = 0; b < fps; b++) {
    blobs[b] = plain_compress(items[b].data(), n, 1);
    bytes += blobs[b].size();
  }
  auto t1 = std::chrono::steady_clock::now();
  size_t wrong = 0;
  for (size_t b = 0; b < fps; b++) {
    Items back;
    int algorithm;
    if (plain_decompress(blobs[b], &back, &algorithm) != 0 || back != items[b]) wrong++;
  }
  auto t2 = std::chrono::steady_clock::now();
  std::printf("{\"fingerprints\": %zu, \"items\": %zu, \"blob_bytes\": %zu, \"compress_s\": %.6f, \"decompress_s\": %.6f, \"wrong\": %zu}\n", fps, n,
              bytes, std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(t2 - t1).count(), wrong);
  return wrong ? 1 : 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && std::string(argv[1]) == "bench") return run_bench((size_t)std::atoll(argv[2]), (size_t)std::atoll(argv[3]));
  return run_checks();
}
