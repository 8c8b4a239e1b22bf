// libneedle_chromaprint.so: libchromaprint's streaming C API (the part needle uses) over the streaming GPU
// fingerprinter: a context owns a one-lane feeder (needle_hip_feeder_*), chromaprint_feed gathers at most one block of
// PCM on the host (4 s; NEEDLE_CHROMAPRINT_FEED_BLOCK: samples per channel) and feeds every full block,
// chromaprint_finish flushes.  The compressed forms (chromaprint_get_fingerprint, _encode_fingerprint, _decode_fingerprint)
// go through the device codec (needle_hip_fingerprint_*, needle_hip_feeder_compressed).  See include/needle_chromaprint.h.
#include "../../include/needle_chromaprint.h"

#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/needle_hip.h"

struct ChromaprintContextPrivate {
  int algorithm = CHROMAPRINT_ALGORITHM_DEFAULT;
  int channels = 1;
  int rate = 11025;
  bool started = false, finished = false;
  bool cleared = false;            // chromaprint_clear_fingerprint since finish()
  NeedleHipFeeder *feeder = nullptr;
  size_t block_frames = 0;         // samples per channel gathered before they go to the feeder
  std::vector<int16_t> block;      // at most that many, not yet fed
  std::vector<uint32_t> raw;       // raw fingerprint after finish()
  ~ChromaprintContextPrivate() { needle_hip_feeder_free(feeder); }
  bool flush() {
    if (block.empty()) return true;
    const void *ptrs[1] = {block.data()};
    const size_t lens[1] = {block.size()};
    const bool ok = needle_hip_feeder_feed(feeder, ptrs, lens) == NeedleError_Ok;
    block.clear();
    return ok;
  }
};

extern "C" {

const char *chromaprint_get_version(void) { return "1.5.1-needle-hip"; }

ChromaprintContext *chromaprint_new(int algorithm) {
  if (algorithm != CHROMAPRINT_ALGORITHM_TEST2) return nullptr;  // the only algorithm needle uses (Context::default)
  ChromaprintContext *ctx = new (std::nothrow) ChromaprintContextPrivate();
  if (ctx) ctx->algorithm = algorithm;
  return ctx;
}

void chromaprint_free(ChromaprintContext *ctx) { delete ctx; }
int chromaprint_get_algorithm(ChromaprintContext *ctx) { return ctx ? ctx->algorithm : -1; }
int chromaprint_get_num_channels(ChromaprintContext *) { return 1; }  // channels of the internal (mono) signal
int chromaprint_get_sample_rate(ChromaprintContext *) { return needle_hip_fingerprint_sample_rate(); }
int chromaprint_get_item_duration(ChromaprintContext *) { return 1365; }
int chromaprint_get_item_duration_ms(ChromaprintContext *) { return needle_hip_fingerprint_item_duration_ms(); }
int chromaprint_get_delay(ChromaprintContext *) { return (4 + 15) * 1365 + (4096 - 1365); }
int chromaprint_get_delay_ms(ChromaprintContext *) { return needle_hip_fingerprint_delay_ms(); }

int chromaprint_start(ChromaprintContext *ctx, int sample_rate, int num_channels) {
  if (!ctx) return 0;
  // needle feeds chromaprint's own 11025 Hz (analyzer.rs:179-187); any other rate goes through the device
  // resampler first, as libchromaprint's internal resampler would
  if (sample_rate < 2000 || sample_rate > 768000) return 0;
  if (num_channels != 1 && num_channels != 2) return 0;
  needle_hip_feeder_free(ctx->feeder);
  ctx->feeder = nullptr;
  if (needle_hip_feeder_new(1, num_channels, sample_rate, NEEDLE_HIP_SAMPLE_S16, 1, &ctx->feeder) != NeedleError_Ok) return 0;
  ctx->channels = num_channels;
  ctx->rate = sample_rate;
  ctx->block_frames = 4 * (size_t)sample_rate;
  if (const char *e = std::getenv("NEEDLE_CHROMAPRINT_FEED_BLOCK")) ctx->block_frames = (size_t)std::atoll(e) > 0 ? (size_t)std::atoll(e) : 1;
  ctx->block.clear();
  ctx->raw.clear();
  ctx->started = true;
  ctx->finished = false;
  ctx->cleared = false;
  return 1;
}

int chromaprint_feed(ChromaprintContext *ctx, const int16_t *data, int size) {
  if (!ctx || !ctx->started || ctx->finished || size < 0 || (size && !data)) return 0;
  if (size % ctx->channels != 0) return 0;
  try {
    const size_t cap = ctx->block_frames * (size_t)ctx->channels;
    size_t left = (size_t)size;
    while (left) {
      const size_t take = left < cap - ctx->block.size() ? left : cap - ctx->block.size();
      ctx->block.insert(ctx->block.end(), data, data + take);
      data += take;
      left -= take;
      if (ctx->block.size() == cap && !ctx->flush()) return 0;
    }
  } catch (...) {
    return 0;
  }
  return 1;
}

int chromaprint_finish(ChromaprintContext *ctx) {
  if (!ctx || !ctx->started) return 0;
  if (ctx->finished) return 1;
  try {
    if (!ctx->flush() || needle_hip_feeder_finish(ctx->feeder, nullptr, 0) != NeedleError_Ok) return 0;
    size_t n = 0;
    if (needle_hip_feeder_ready(ctx->feeder, 0, &n, nullptr, nullptr) != NeedleError_Ok) return 0;
    ctx->raw.assign(n ? n : 1, 0);
    if (needle_hip_feeder_items(ctx->feeder, 0, 0, n, ctx->raw.data()) != NeedleError_Ok) return 0;
    ctx->raw.resize(n);
    ctx->block.shrink_to_fit();
  } catch (...) {
    return 0;
  }
  ctx->finished = true;
  return 1;
}

int chromaprint_get_raw_fingerprint(ChromaprintContext *ctx, uint32_t **fingerprint, int *size) {
  if (!ctx || !fingerprint || !size || !ctx->finished) return 0;
  uint32_t *out = static_cast<uint32_t *>(std::malloc(sizeof(uint32_t) * (ctx->raw.size() ? ctx->raw.size() : 1)));
  if (!out) return 0;
  if (!ctx->raw.empty()) std::memcpy(out, ctx->raw.data(), sizeof(uint32_t) * ctx->raw.size());
  *fingerprint = out;
  *size = (int)ctx->raw.size();
  return 1;
}

int chromaprint_get_raw_fingerprint_size(ChromaprintContext *ctx, int *size) {
  if (!ctx || !size || !ctx->finished) return 0;
  *size = (int)ctx->raw.size();
  return 1;
}

int chromaprint_clear_fingerprint(ChromaprintContext *ctx) {
  if (!ctx) return 0;
  ctx->raw.clear();
  ctx->cleared = true;
  return 1;
}

// a malloc'd copy the caller frees with chromaprint_dealloc; bytes from this library's own allocator are released here
static void *take(void *from, size_t n, size_t extra) {
  void *out = std::malloc(n + extra ? n + extra : 1);
  if (out && n) std::memcpy(out, from, n);
  if (out && extra) std::memset(static_cast<char *>(out) + n, 0, extra);
  needle_hip_host_free(from);
  return out;
}

// blob -> *encoded (NUL-terminated either way), base64 or as it is
static int hand_over(uint8_t *blob, size_t size, int base64, char **encoded, int *encoded_size) {
  if (!base64) {
    *encoded = static_cast<char *>(take(blob, size, 1));
    if (encoded_size) *encoded_size = (int)size;
    return *encoded != nullptr;
  }
  char *text = nullptr;
  size_t text_size = 0;
  const bool ok = needle_hip_fingerprint_base64_encode(blob, size, &text, &text_size) == NeedleError_Ok;
  needle_hip_host_free(blob);
  if (!ok) return 0;
  *encoded = static_cast<char *>(take(text, text_size, 1));
  if (encoded_size) *encoded_size = (int)text_size;
  return *encoded != nullptr;
}

int chromaprint_get_fingerprint(ChromaprintContext *ctx, char **fingerprint) {
  if (!ctx || !fingerprint || !ctx->finished || ctx->cleared) return 0;
  uint8_t *blob = nullptr;
  size_t size = 0;
  if (needle_hip_feeder_compressed(ctx->feeder, 0, ctx->algorithm, &blob, &size) != NeedleError_Ok) return 0;
  return hand_over(blob, size, 1, fingerprint, nullptr);
}

int chromaprint_get_fingerprint_hash(ChromaprintContext *ctx, uint32_t *hash) {
  if (!ctx || !hash || !ctx->finished) return 0;
  return needle_hip_fingerprint_simhash(ctx->raw.data(), ctx->raw.size(), hash) == NeedleError_Ok;
}

int chromaprint_encode_fingerprint(const uint32_t *fp, int size, int algorithm, char **encoded_fp, int *encoded_size, int base64) {
  if (size < 0 || (size && !fp) || !encoded_fp || !encoded_size) return 0;
  const uint64_t item_off[2] = {0, (uint64_t)size};
  uint64_t blob_off[2] = {0, 0};
  uint8_t *blob = nullptr;
  if (needle_hip_fingerprint_compress_host(fp, item_off, 1, algorithm, &blob, blob_off) != NeedleError_Ok) return 0;
  return hand_over(blob, (size_t)blob_off[1], base64, encoded_fp, encoded_size);
}

int chromaprint_decode_fingerprint(const char *encoded_fp, int encoded_size, uint32_t **fp, int *size, int *algorithm, int base64) {
  if (encoded_size < 0 || (encoded_size && !encoded_fp) || !fp || !size) return 0;
  uint8_t *bytes = nullptr;
  size_t n = (size_t)encoded_size;
  if (base64 && needle_hip_fingerprint_base64_decode(encoded_fp, (size_t)encoded_size, &bytes, &n) != NeedleError_Ok) return 0;
  const uint64_t blob_off[2] = {0, n};
  uint64_t item_off[2] = {0, 0};
  uint32_t *items = nullptr;
  int32_t alg = 0, status = 0;
  const bool ok = needle_hip_fingerprint_decompress_host(base64 ? bytes : reinterpret_cast<const uint8_t *>(encoded_fp), blob_off, 1, &items,
                                                         item_off, &alg, &status) == NeedleError_Ok;
  needle_hip_host_free(bytes);
  if (!ok) return 0;
  if (status != 0) {  // refused: shorter than a header, a stream that ends early, a bit position above 32
    needle_hip_host_free(items);
    return 0;
  }
  *fp = static_cast<uint32_t *>(take(items, (size_t)item_off[1] * sizeof(uint32_t), 0));
  if (!*fp) return 0;
  *size = (int)item_off[1];
  if (algorithm) *algorithm = alg;
  return 1;
}

int chromaprint_hash_fingerprint(const uint32_t *fp, int size, uint32_t *hash) {
  if (size < 0 || (size && !fp) || !hash) return 0;
  return needle_hip_fingerprint_simhash(fp, (size_t)size, hash) == NeedleError_Ok;
}

void chromaprint_dealloc(void *ptr) { std::free(ptr); }

}  // extern "C"
