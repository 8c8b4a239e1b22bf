// libneedle_chromaprint.so: libchromaprint's streaming C API (the part needle uses) over the streaming GPU
// fingerprinter: a context owns a one-lane feeder (needle_hip_feeder_*), chromaprint_feed gathers at most one block of
// PCM on the host (4 s; NEEDLE_CHROMAPRINT_FEED_BLOCK: samples per channel) and feeds every full block,
// chromaprint_finish flushes.  See include/needle_chromaprint.h.
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
  return 1;
}

void chromaprint_dealloc(void *ptr) { std::free(ptr); }

}  // extern "C"
