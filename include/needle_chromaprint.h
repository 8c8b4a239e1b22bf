/*
 * needle_chromaprint.h -- the part of libchromaprint's C API that the MI355X fingerprinter serves: the subset needle
 * reaches through chromaprint-rust 0.1.3 / chromaprint-sys-next 1.5.3 (needle/Cargo.lock:147-161), and the fingerprint
 * codec.  Call sites in the reference: needle/src/audio/analyzer.rs:176 (chromaprint_new), :179
 * (chromaprint_get_sample_rate), :218 (chromaprint_start), :275 (chromaprint_feed), :286 (chromaprint_finish),
 * :288 (chromaprint_get_delay_ms), :289 (chromaprint_get_item_duration_ms), :300
 * (chromaprint_get_raw_fingerprint + chromaprint_dealloc).
 *
 * Exported by libneedle_chromaprint.so with libchromaprint's own symbol names, so a needle built with
 * CHROMAPRINT_SYS_DYNAMIC (README.md:209) -- or any program written against libchromaprint -- can be pointed at it
 * instead of libchromaprint and runs its analyze step on the GPU without source changes.  feed() gathers PCM a block at
 * a time and streams it through a one-lane needle_hip_feeder; finish() flushes.  Conventions are libchromaprint's:
 * every int function returns 1 on success and 0 on error.  The fingerprinter itself supports only
 * CHROMAPRINT_ALGORITHM_TEST2 (the default) and 1-2 channels; any sample rate is resampled on the device.
 *
 * The codec: chromaprint_get_fingerprint gives the compressed, base64 string `fpcalc` prints (0 before finish() and
 * after chromaprint_clear_fingerprint); chromaprint_encode_fingerprint / chromaprint_decode_fingerprint convert between
 * raw items and the compressed form, binary or base64 (URL-safe, unpadded), for ANY algorithm byte -- it is only a label
 * there; decode returns 0 for a blob it refuses (shorter than a header, a stream that ends early, a bit position above
 * 32); chromaprint_get_fingerprint_hash / chromaprint_hash_fingerprint are the 32-bit simhash (0 for an empty
 * fingerprint).  Every result is malloc'd, NUL-terminated where it is text, and freed with chromaprint_dealloc.  The
 * codec runs on the device (include/needle_hip.h, needle_hip_fingerprint_*).
 */
#ifndef NEEDLE_CHROMAPRINT_H
#define NEEDLE_CHROMAPRINT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ChromaprintContextPrivate ChromaprintContext;

enum ChromaprintAlgorithm {
  CHROMAPRINT_ALGORITHM_TEST1 = 0,
  CHROMAPRINT_ALGORITHM_TEST2,
  CHROMAPRINT_ALGORITHM_TEST3,
  CHROMAPRINT_ALGORITHM_TEST4,
  CHROMAPRINT_ALGORITHM_TEST5,
  CHROMAPRINT_ALGORITHM_DEFAULT = CHROMAPRINT_ALGORITHM_TEST2
};

const char *chromaprint_get_version(void);
ChromaprintContext *chromaprint_new(int algorithm);
void chromaprint_free(ChromaprintContext *ctx);
int chromaprint_get_algorithm(ChromaprintContext *ctx);
int chromaprint_get_num_channels(ChromaprintContext *ctx);
int chromaprint_get_sample_rate(ChromaprintContext *ctx);
int chromaprint_get_item_duration(ChromaprintContext *ctx);    /* samples: 1365 */
int chromaprint_get_item_duration_ms(ChromaprintContext *ctx); /* 123 */
int chromaprint_get_delay(ChromaprintContext *ctx);            /* samples: 28666 */
int chromaprint_get_delay_ms(ChromaprintContext *ctx);         /* 2600 */
int chromaprint_start(ChromaprintContext *ctx, int sample_rate, int num_channels);
int chromaprint_feed(ChromaprintContext *ctx, const int16_t *data, int size);
int chromaprint_finish(ChromaprintContext *ctx);
int chromaprint_get_raw_fingerprint(ChromaprintContext *ctx, uint32_t **fingerprint, int *size);
int chromaprint_get_raw_fingerprint_size(ChromaprintContext *ctx, int *size);
int chromaprint_clear_fingerprint(ChromaprintContext *ctx);
int chromaprint_get_fingerprint(ChromaprintContext *ctx, char **fingerprint);
int chromaprint_get_fingerprint_hash(ChromaprintContext *ctx, uint32_t *hash);
int chromaprint_encode_fingerprint(const uint32_t *fp, int size, int algorithm, char **encoded_fp, int *encoded_size, int base64);
int chromaprint_decode_fingerprint(const char *encoded_fp, int encoded_size, uint32_t **fp, int *size, int *algorithm, int base64);
int chromaprint_hash_fingerprint(const uint32_t *fp, int size, uint32_t *hash);
void chromaprint_dealloc(void *ptr);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLE_CHROMAPRINT_H */
