/*
 * needle_hip.h — additive, GPU-facing entry points of libneedle_capi.so (MI355X / gfx950).
 *
 * needle.h is the reference's C ABI verbatim; it only moves file paths.  The reference's hot path,
 * however, runs *below* that surface, inside `Analyzer::process_frames` (chromaprint feed/finish,
 * needle/src/audio/analyzer.rs:176-300) and `Comparator::longest_common_hash_match`
 * (needle/src/audio/comparator.rs:157-250).  The functions here are the C-ABI form of exactly those
 * two inner interfaces plus the in-memory calls the Rust API has and the C API lacks
 * (`Comparator::run_with_frame_hashes`, comparator.rs:524; `FrameHashes` accessors, data.rs:143-168 —
 * needle-capi/src/lib.rs:306-314 wraps FrameHashes as an opaque "TODO").  Plain pointers and sizes,
 * no C++/torch types.  All functions return NeedleError; details of the last failure on the calling
 * thread are available from needle_hip_last_error_message().
 *
 * Nothing here has a CPU fallback: without a usable HIP device the compute entry points fail with
 * NeedleError_Unknown ("no HIP device").
 */
#ifndef NEEDLE_HIP_H
#define NEEDLE_HIP_H

#include "needle.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device / diagnostics ------------------------------------------------------------------------ */
enum NeedleError needle_hip_device_count(int *count);
enum NeedleError needle_hip_set_device(int ordinal);
enum NeedleError needle_hip_synchronize(void);
/* PCI address of the current device, "0000:c1:00.0" form (NUL-terminated): lets a host program find the device's
 * sysfs node (clocks, temperature) without HIP headers.  Diagnostics only. */
enum NeedleError needle_hip_device_pci_bus_id(char out[32]);
/* The HIP stream (a hipStream_t) every kernel and copy of this library is enqueued on, for the current device:
 * lets a caller order its own device work (collectives, framework kernels) against the library's by stream
 * order or events instead of host synchronisation.  NULL without a device. */
void *needle_hip_stream(void);
const char *needle_hip_last_error_message(void);
const char *needle_hip_version(void);

/* Thin device-memory helpers so a host program (Rust/C/Python) needs no HIP headers. */
enum NeedleError needle_hip_malloc(void **device_ptr, size_t bytes);
enum NeedleError needle_hip_free(void *device_ptr);
enum NeedleError needle_hip_memcpy_h2d(void *device_dst, const void *host_src, size_t bytes);
enum NeedleError needle_hip_memcpy_d2h(void *host_dst, const void *device_src, size_t bytes);
void needle_hip_host_free(void *ptr); /* frees arrays this library malloc'd for the caller */
/* Pinned (page-locked) host memory for PCM the caller wants uploaded at the full PCIe rate without staging. */
enum NeedleError needle_hip_host_alloc(void **host_ptr, size_t bytes);
enum NeedleError needle_hip_host_alloc_free(void *host_ptr);

/* GPU timing of the most recent COMPLETED launch of a kernel (it never waits behind queued work unless no
 * launch has finished yet), measured with HIP events on the
 * library's own stream (rocprofv3 sees the same kernels).  Names: "stft_chroma", "fir_norm",
 * "classify", "hamming_runs", "simhash_runs", "resample", "downmix", "convert".  Returns milliseconds, <0 if unknown or
 * not timed. */
double needle_hip_last_kernel_ms(const char *kernel);
/* Selects the kernels that get those events: "all", a comma-separated list of names, or NULL / "" / "none".
 * Default: none (each event record is one more packet between dependent dispatches: timing all five kernels of
 * a 28 x 24 min job costs 3 % of its time), unless the environment variable NEEDLE_HIP_KERNEL_TIMING is set.
 * With the extra item "sum" (e.g. "all,sum") every launch since this call keeps its own events and
 * needle_hip_last_kernel_ms returns their SUM (it waits for them): a kernel that one job launches several times -- the
 * first pass of a library-scale job -- then reads as the job's total, not as its last launch's. */
void needle_hip_set_kernel_timing(const char *kernels);
/* With "sum": the launches of that name that have been given events since the last needle_hip_set_kernel_timing call;
 * otherwise, and for an unknown name, 0.  Only the first 4096 launches of a name keep events: the count stops there, so a
 * reader that may see more sets the selection again in between.  Further names: "ingest", "rematrix", "feeder_carry". */
size_t needle_hip_kernel_launches(const char *kernel);
/* Diagnostic for the search roofline: table cells per second this device sustains on the scan's
 * per-cell instruction sequence (xor, popcount, compare, select) with operands in registers -- the integer-VALU
 * ceiling a brute-force evaluation of every cell of comparator.rs:176-187 cannot exceed.  Takes ~10 ms. */
enum NeedleError needle_hip_int_valu_ceiling(double *cells_per_second);
/* The other half of that roofline.  The fast scan does not evaluate every cell of the table: a run of >= min_len must
 * cover an aligned 8-row window, so only those rows are looked at, and most windows are abandoned after three of them.
 * With NEEDLE_HIP_SCAN_COUNT=1 in the environment every scan launch runs a COUNTING instantiation of the same kernel
 * (slower; never time it) that adds up the cell evaluations it ISSUES -- xor / popcount / compare over a wave's 64
 * lanes, inside the table or not.  This returns the sum since the last reset (waits for the library stream):
 * issued evaluations per second of the UNCOUNTED kernel against needle_hip_int_valu_ceiling() is a fraction <= 1. */
enum NeedleError needle_hip_scan_issued_evaluations(uint64_t *lane_evaluations, bool reset);
/* The same counting launches, two figures: counts[0] = the issued lane evaluations above, counts[1] = diagonals that
 * passed the head rows of a window (summed over all windows) and had to be finished -- what a cheaper head costs.  The
 * window shape itself (rows per aligned window W, head rows H; default 8, 3) can be chosen among the instantiated ones
 * with NEEDLE_HIP_SCAN_SHAPE="W,H" (W in 4, 8, 16; H in 2..4): every shape emits the same runs (tools/scan_shape_sweep.py). */
enum NeedleError needle_hip_scan_counts(uint64_t counts[2], bool reset);
/* Which form of the scan the last launch of this process took: 0 none yet, 1 one lane per diagonal (short minimum runs),
 * 2 bands, 3 aligned windows on the vector ALU, 4 aligned windows with the head rows on the matrix pipe (launches of 2048
 * sequence pairs or more, thresholds <= 15, windows that fill their row tiles; NEEDLE_HIP_SCAN_MFMA=0 / 1 forces either)
 * -- and for form 4 the v_mfma_f32_32x32x64_f8f6f4 instructions (FP4 operands, two head rows each) that launch issued
 * (131 072 operations each): the numerator of ITS roofline.  Every form emits the same runs. */
enum NeedleError needle_hip_scan_last_launch(int32_t *form, uint64_t *matrix_products);
/* How many jobs of this process asked for the per-video epilogue (comparator.rs:405-515, 583-626) on the DEVICE and were
 * handed back to the host form because one pair's bucket of runs exceeded what the device orders (since round 6 a
 * bucket beyond a lane's 24 runs is a workgroup's, up to 8192 runs: two fully silent 24-minute windows are 5 800;
 * beyond that, or with a row of 65 536 hashes or more).  Correct either way; this makes the performance cliff
 * visible (also printed under NEEDLE_HIP_TRACE).  reset: start counting again. */
enum NeedleError needle_hip_epilogue_host_fallbacks(uint64_t *jobs, bool reset);

/* ---- fingerprint: the chromaprint Context replacement -------------------------------------------
 * Replaces chromaprint::Context::{start,feed,finish,get_fingerprint_raw,get_delay,get_item_duration,
 * sample_rate} as called from analyzer.rs:176,179,218,275,286,288-289,300.  Batched: many streams
 * per call.  PCM is interleaved s16 at needle_hip_fingerprint_sample_rate() Hz, `channels` = 1 to
 * NEEDLE_HIP_MAX_CHANNELS in needle_hip_fingerprint_host (the reference always feeds 2, analyzer.rs:218; stereo is
 * down-mixed (L+R)/2 with C truncation on the device, 3-8 channels by needle_hip_downmix_host's arithmetic), 1 or 2
 * in the _device, _audit_device and _debug forms.  `step` keeps raw items 0, step, 2*step, ... (analyzer.rs:293-304; step = 1 returns
 * chromaprint's full raw fingerprint). */
#define NEEDLE_HIP_MAX_CHANNELS 8                 /* interleaved channels the analyze paths accept (1..8) */
int needle_hip_fingerprint_sample_rate(void);      /* 11025 */
int needle_hip_fingerprint_delay_ms(void);         /* 2600  (chromaprint_get_delay_ms) */
int needle_hip_fingerprint_item_duration_ms(void); /* 123   (chromaprint_get_item_duration_ms) */
size_t needle_hip_fingerprint_num_items(size_t samples_per_channel);
size_t needle_hip_fingerprint_num_kept(size_t samples_per_channel, uint32_t step);

/* Host buffers in, host buffers out (does H2D/D2H).  items[i] must hold num_kept(...) values. */
enum NeedleError needle_hip_fingerprint_host(const int16_t *const *pcm, const size_t *num_values,
                                             size_t num_streams, int channels, uint32_t step,
                                             uint32_t *const *items);

/* PCM already resident in HBM: stream i is d_pcm[pcm_offsets[i] .. +num_values[i]) (offsets in s16
 * values, host arrays); kept items of stream i are written to d_items[item_offsets[i] ..].  Runs on
 * the library stream; returns after the kernels are enqueued unless `sync` is true. */
enum NeedleError needle_hip_fingerprint_device(const int16_t *d_pcm, const uint64_t *pcm_offsets,
                                               const uint64_t *num_values, size_t num_streams,
                                               int channels, uint32_t step, uint32_t *d_items,
                                               const uint64_t *item_offsets, bool sync);

/* Arithmetic of the fingerprinter.  The u32 items are DEFINED on a double-precision pipeline (chromaprint on an f64
 * FFT; oracle/ora_chromaprint.c).  By default the STFT runs a single-precision first pass and every item is either
 * certified -- all 48 threshold comparisons clear a data-dependent error radius, so the f64 pipeline provably takes the
 * same decisions -- or recomputed: the frames it covers go through the f64 kernel again and the item is classified
 * from those.  The emitted items are therefore the f64 pipeline's, bit for bit.  Environment: NEEDLE_HIP_STFT=f64 runs
 * the f64 kernel over everything; NEEDLE_HIP_CERT_K scales the radius (default 64; 0 accepts every first-pass item,
 * for tests).  counts = {items fingerprinted, items recomputed in f64, chunks of 2 frame pairs, chunks recomputed}
 * on the current device since the last reset; waits for the library stream. */
enum NeedleError needle_hip_fingerprint_cert_stats(uint64_t counts[4], bool reset);

/* Audit of that first pass.  The acceptance radius is an EMPIRICAL guard, not a proven bound: K = 64
 * times the error scale S, where the worst |log v32 - log v64| / S ever observed is 1.8.  This makes the claim checkable on
 * any input: both transforms -- the f32 first pass and the f64 kernel -- run over the same resident PCM into buffers of
 * their own and every kept item is examined on the device with the certification kernel's own functions and K.
 *   items                : kept items examined
 *   accepted             : items the first pass accepted (emitted from f32 chroma)
 *   accepted_mismatches  : accepted items whose f32 bits differ from the f64 pipeline's item (each one a hole: must be 0)
 *   mismatches           : items of `d_items` (what the product emitted for these streams) that differ from the f64 item
 *   max_error_over_s     : max over accepted items and their 16 classifiers of |log v32 - log v64| / S (compare with K)
 *   max_s                : largest S among accepted items
 * Same stream description as needle_hip_fingerprint_device; synchronous; allocates 2 x 96 B per frame while it runs. */
typedef struct NeedleHipCertAudit {
  uint64_t items, accepted, accepted_mismatches, mismatches;
  double max_error_over_s, max_s;
} NeedleHipCertAudit;
enum NeedleError needle_hip_fingerprint_audit_device(const int16_t *d_pcm, const uint64_t *pcm_offsets,
                                                     const uint64_t *num_values, size_t num_streams, int channels,
                                                     uint32_t step, const uint32_t *d_items, const uint64_t *item_offsets,
                                                     NeedleHipCertAudit *audit);

/* Test hook: intermediate stages of one stream, copied to the host.  chroma [frames][12] (energy per
 * pitch class per FFT frame), features [frames-4][12] (FIR-filtered, L2-normalised). NULLs allowed. */
enum NeedleError needle_hip_fingerprint_debug(const int16_t *pcm, size_t num_values, int channels,
                                              double *chroma, double *features);

/* Test hook: what each of the four kernels of the certified chain wrote (f32 first pass -> certification -> f64
 * recomputation of the listed chunks -> fix-up of the listed items), copied to the host.  Host PCM streams as
 * needle_hip_fingerprint_host takes them; the hook runs the product's own chain over them as ONE batch -- the same
 * planning, launch sizes, schedule and kernels as needle_hip_fingerprint_device, with device-to-device copies between
 * the launches -- after filling the chain's chroma and energy rows with a NaN bit pattern (bytes 0xFF), so that a row no
 * kernel wrote shows.  Differences from the product's call: a batch without one kept item still runs its first pass,
 * and flags bit 0 picks the recomputation kernel's "beside" form (the one pipelined library jobs use).
 * NEEDLE_HIP_CERT_K, NEEDLE_STFT_PAIRS and NEEDLE_HIP_ITEMS_PER_TILE act as in the product; NEEDLE_HIP_STFT=f64 (no
 * chain to look at) and a batch the product would cut into more than one chunk are refused with InvalidArgument.
 * Frames, pairs, chunks and items are numbered over the whole batch, stream after stream; streams[i] says where stream
 * i's begin.  Any output pointer may be NULL.  A batch without a frame launches nothing and reports zeros. */
typedef struct NeedleHipStageStream {
  uint32_t frames, frame_base; /* rows [frame_base, frame_base + frames) of the chroma and energy outputs */
  uint32_t pair_base;          /* its frame pairs: [pair_base, pair_base + ceil(frames / 2)); pair p is in chunk p / chunk_pairs */
  uint32_t kept, kept_base;    /* its kept items: [kept_base, kept_base + kept); item k starts at the stream's frame k * step */
  uint32_t tile_base;          /* its tiles of items_per_tile items in the certification's launch */
} NeedleHipStageStream;
typedef struct NeedleHipStages {
  /* in: where to copy (NULL: not wanted) */
  double *first_chroma;   /* [frames][12]: the first pass's rows (f32 values held as doubles), before the certification */
  float *energy;          /* [frames][4]: its energy partials; both frames of a pair carry the pair's */
  uint32_t *first_items;  /* [kept]: as the certification wrote them, before the fix-up */
  uint8_t *item_listed;   /* [kept]: times the item is in the list of refused items (0 or 1) */
  uint8_t *chunk_listed;  /* [chunks] (room for max(pairs, 1) always suffices): times the chunk is in the list (0 or 1) */
  double *final_chroma;   /* [frames][12]: after the recomputation */
  uint32_t *items;        /* [kept]: after the fix-up, what the product emits */
  NeedleHipStageStream *streams; /* [num_streams] */
  /* out */
  uint64_t frames, pairs, kept, chunks;
  uint64_t items_listed, chunks_listed;      /* the certification's own counters */
  uint32_t chunk_pairs, items_per_tile;
  uint32_t compute_units, pairs_per_block;   /* of the device; of the first pass's launch */
  uint32_t pairs_per_xcd, blocks_per_xcd;    /* the first pass's schedule: every XCD walks its part of the pairs in */
  uint32_t block_size[4], block_count[4];    /* block_count[k] workgroups of block_size[k] pairs, k = 0..3 in turn */
} NeedleHipStages;
enum NeedleError needle_hip_fingerprint_stages_debug(const int16_t *const *pcm, const size_t *num_values, size_t num_streams,
                                                     int channels, uint32_t step, uint32_t flags, NeedleHipStages *stages);

/* ---- resampler + down-mix: the step in FRONT of the path ---------------------------------------------
 * The reference converts decoded audio to s16 @ 11025 Hz with FFmpeg's swresample before feeding chromaprint
 * (analyzer.rs:180-187,231-282).  That library is out of scope and not bit-reproducible; this front-end is this
 * project's own specification (integer down-mix, rational polyphase Kaiser-sinc FIR, f32 fused multiply-adds
 * in tap order, round to nearest even; oracle/ora_resample.h) so that PCM at the usual decode rates can be
 * analysed on the device.  Output: mono s16 at 11025 Hz, ceil(n * 11025 / rate) samples per stream.
 * needle_audio_analyzer_run and needle_hip_analyzer_run_pcm apply it automatically when the rate differs. */
size_t needle_hip_resample_out_len(size_t samples_per_channel, int sample_rate);
enum NeedleError needle_hip_resample_host(const int16_t *const *pcm, const size_t *num_values, size_t num_streams,
                                          int channels, int sample_rate, int16_t *const *out);
/* Which kernel resamples PCM at `sample_rate`, and its geometry: what the launch itself reads, so a test can say which
 * kernel it covers.  Host arithmetic only -- no device is touched and no coefficient is designed.  The tuning switches of
 * the environment (NEEDLE_HIP_RESAMPLE_V1, _QUAD, _SPLITS) are honoured as the launch honours them.  A rate these kernels
 * cannot take (its ratio to 11025 Hz in lowest terms is too large: resample to a rate that shares a larger factor with
 * 11025 first) gives NeedleError_InvalidArgument with family REFUSED and L, M, T filled; a rate outside 2000..768000
 * gives NeedleError_InvalidArgument and leaves *out zeroed.  Fields that do not apply to the family are 0. */
enum NeedleHipResampleFamily {
  NEEDLE_HIP_RESAMPLE_IDENTITY = 0, /* 11025 Hz: the general kernel with a single unit tap */
  NEEDLE_HIP_RESAMPLE_DEC = 1,      /* integer decimation by 2 or 4, scalar coefficients */
  NEEDLE_HIP_RESAMPLE_MFMA = 2,     /* matrix-core kernel */
  NEEDLE_HIP_RESAMPLE_QUAD = 3,     /* four outputs per lane, DPP operands */
  NEEDLE_HIP_RESAMPLE_GENERAL = 4,  /* one output per lane */
  NEEDLE_HIP_RESAMPLE_REFUSED = 5
};
typedef struct NeedleHipResamplePlan {
  int family;          /* enum NeedleHipResampleFamily */
  int L, M, T;         /* 11025 / rate = L / M in lowest terms, T taps per output */
  int tile_outputs;    /* consecutive outputs of a stream per tile */
  int blocks_per_tile; /* workgroups a tile is cut into */
  int threads;         /* per workgroup */
  int lds_bytes;       /* dynamic LDS of the launch (dec: its static LDS is not counted) */
  /* general kernel (and identity) */
  int n;               /* lanes per phase */
  int row_mode;        /* 1: the region is n rows, 0: contiguous */
  int rows_in_lds;     /* 1: coefficient rows through a per-wave LDS scratch, 0: straight from global memory */
  int vec4;            /* general and quad: M % 4 == 0, staging by aligned groups of four */
  int groups;          /* G: 16-byte groups per shifted coefficient row */
  int pitch;           /* general (row mode) and quad: 16-byte slots per row of samples */
  int region_slots;    /* general: 16-byte slots of samples */
  int delta;           /* samples the region starts before a tile's first tap, so that it starts at a multiple of 4 */
  /* matrix-core kernel */
  int mfma_steps;      /* 12, 20, 36 or 52: the kernel's STEPS */
  int nblocks;         /* blocks of sixteen outputs per row */
  int mf_splits, mf_waves, mf_groups;
  int mf_long_row;     /* 1: a row is longer than the groups its staging threads move (dup_lo, dup_hi in use) */
  int mf_dup_lo, mf_dup_hi;
  /* quad kernel */
  int quad_splits, quads_per_split, quad_threads;
  int quad_rounds;     /* rounds of quads a workgroup makes */
  int quad_small;      /* 1: the instantiations for at most 640 threads */
  int quad_steps;      /* 16-byte groups of a row a quad multiplies */
  int dec_q;           /* dec: outputs per lane */
} NeedleHipResamplePlan;
enum NeedleError needle_hip_resample_plan(int sample_rate, NeedleHipResamplePlan *out);
/* The down-mix on its own (`channels` = 1..NEEDLE_HIP_MAX_CHANNELS): out[i][n] = (sum of the `channels` values of frame n
 * of pcm[i]) / channels, C integer division (truncation toward zero); out[i] must hold num_values[i] / channels values
 * (a trailing partial frame is dropped).  Every analyze path applies it on the device to 3-8 channel input before the
 * resampler and the fingerprinter; 1 and 2 channels keep their own paths. */
enum NeedleError needle_hip_downmix_host(const int16_t *const *pcm, const size_t *num_values, size_t num_streams,
                                         int channels, int16_t *const *out);

/* ---- sample formats: PCM as a decoder hands it over, converted to s16 on the device -------------------
 * The values follow FFmpeg's AVSampleFormat numbering, so a caller can pass frame->format through.  Interleaved
 * formats take one pointer per stream; planar ones take one pointer per CHANNEL: the pointer array then has
 * num_streams * channels entries and pcm[i * channels + c] is plane c of stream i, holding num_values[i] / channels
 * samples.  num_values[i] counts samples over all channels (frames x channels) whatever their width; a trailing
 * partial frame is dropped.  Pointers need only the alignment of one sample.  Conversion of one sample to s16 (the WAV
 * reader's arithmetic, so a WAV file and its raw samples give the same hashes):
 *   U8 : (x - 128) << 8        S16: x        S32: x >> 16 (arithmetic shift)
 *   F32: rint(x * 32768.0f) in f32, ties to even; NaN gives 0; otherwise clipped to [-32768, 32767]
 *   F64: the same in f64 (it never passes through f32)
 * Everything behind the conversion is the s16 path on the converted values: every result equals, bit for bit, what the
 * s16 entry point gives for the host-converted, interleaved samples.  Any other value: NeedleError_InvalidArgument. */
enum NeedleHipSampleFormat {
  NEEDLE_HIP_SAMPLE_U8 = 0,
  NEEDLE_HIP_SAMPLE_S16 = 1, /* what every entry point without a format takes, and the default everywhere */
  NEEDLE_HIP_SAMPLE_S32 = 2,
  NEEDLE_HIP_SAMPLE_F32 = 3,
  NEEDLE_HIP_SAMPLE_F64 = 4,
  NEEDLE_HIP_SAMPLE_U8P = 5, /* planar: one plane per channel */
  NEEDLE_HIP_SAMPLE_S16P = 6,
  NEEDLE_HIP_SAMPLE_S32P = 7,
  NEEDLE_HIP_SAMPLE_F32P = 8,
  NEEDLE_HIP_SAMPLE_F64P = 9
};
/* The conversion on its own: out[i] receives interleaved `channels`-channel s16, num_values[i] / channels * channels
 * values, NOT down-mixed (the analyze paths fuse the down-mix of 3-8 channels into the same kernel). */
enum NeedleError needle_hip_convert_host(const void *const *pcm, const size_t *num_values, size_t num_streams,
                                         int channels, int format, int16_t *const *out);

/* ---- search: the LCS-Hamming DP replacement -------------------------------------------------------
 * Replaces Comparator::longest_common_hash_match's two table sweeps (comparator.rs:175-247).  For a
 * problem (src, dst, min_len) it reports every maximal diagonal run of cells (i >= 1, j >= 1) with
 * popcount(src[i] ^ dst[j]) <= threshold whose length L >= min_len, as (src_end = i, dst_end = j, L)
 * of its last cell — exactly the cells the reference's reverse walk stops at (:196-200) with
 * table[i][j] = L — together with the two chromaprint simhashes the reference computes for such a run
 * (:226-229).  Order of the emitted runs is unspecified; the caller sorts. */
typedef struct NeedleHipSeq {
  uint32_t offset; /* first hash of the sequence inside the hash arena */
  uint32_t len;
} NeedleHipSeq;

typedef struct NeedleHipProblem {
  uint32_t src_seq;
  uint32_t dst_seq;
  uint32_t min_len; /* >= 1 */
  uint32_t tag;     /* copied to NeedleHipRun.problem */
} NeedleHipProblem;

typedef struct NeedleHipRun {
  uint32_t problem;
  uint32_t src_end;
  uint32_t dst_end;
  uint32_t len;
  uint32_t src_match_hash; /* simhash32 of src[src_end-len ..= src_end], L+1 hashes (comparator.rs:149-153,226-229) */
  uint32_t dst_match_hash; /* simhash32 of dst[dst_end-len ..= dst_end] */
} NeedleHipRun;

/* Hash arena resident in HBM; descriptors are host arrays.  Writes at most `capacity` runs to d_runs
 * and the TOTAL number found to *d_count (device).  Synchronous when `sync`. */
enum NeedleError needle_hip_hamming_runs_device(const uint32_t *d_hashes, const NeedleHipSeq *seqs,
                                                size_t num_seqs, const NeedleHipProblem *problems,
                                                size_t num_problems, uint32_t threshold,
                                                NeedleHipRun *d_runs, uint32_t capacity,
                                                uint32_t *d_count, bool sync);

/* Host arrays in, malloc'd run list out (free with needle_hip_host_free). */
enum NeedleError needle_hip_hamming_runs_host(const uint32_t *hashes, size_t num_hashes,
                                              const NeedleHipSeq *seqs, size_t num_seqs,
                                              const NeedleHipProblem *problems, size_t num_problems,
                                              uint32_t threshold, NeedleHipRun **runs, size_t *num_runs);

/* ---- FrameHashes (data.rs) ------------------------------------------------------------------------ */
enum NeedleError needle_hip_frame_hashes_new(const uint32_t *opening_hashes, const uint64_t *opening_ts_ns,
                                             size_t num_opening, const uint32_t *ending_hashes,
                                             const uint64_t *ending_ts_ns, size_t num_ending,
                                             uint64_t hash_duration_ns, const char *md5, FrameHashes **output);
void needle_hip_frame_hashes_free(FrameHashes *frame_hashes);
size_t needle_hip_frame_hashes_len(const FrameHashes *frame_hashes, bool ending);          /* data.rs:143,150 */
enum NeedleError needle_hip_frame_hashes_copy(const FrameHashes *frame_hashes, bool ending, uint32_t *hashes,
                                              uint64_t *ts_ns, size_t capacity);
uint64_t needle_hip_frame_hashes_hash_duration_ns(const FrameHashes *frame_hashes);        /* data.rs:157 */
const char *needle_hip_frame_hashes_md5(const FrameHashes *frame_hashes);                  /* data.rs:164 */
enum NeedleError needle_hip_frame_hashes_read(const char *path, FrameHashes **output);     /* data.rs:104-115 */
enum NeedleError needle_hip_frame_hashes_write(const FrameHashes *frame_hashes, const char *path);
enum NeedleError needle_hip_header_md5(const char *path, char out[33]);                    /* util.rs:99-105 */

/* ---- Analyzer at the PCM boundary -----------------------------------------------------------------
 * Analyzer::run (analyzer.rs:425) with FFmpeg's half of process_frames already done by the caller:
 * pcm[i] is the whole decoded stream of video i, interleaved s16 at `sample_rate` (anything but 11025 Hz is
 * resampled on the device first, see above).  Applies the opening / ending search windows
 * (analyzer.rs:378,390), fingerprints on the GPU, attaches timestamps (:293-318), stores the
 * FrameHashes in the handle (retrieve with needle_audio_analyzer_get_frame_hashes) and persists
 * <video>.needle.dat when `persist`. */
enum NeedleError needle_hip_analyzer_run_pcm(struct NeedleAudioAnalyzer *analyzer, const int16_t *const *pcm,
                                             const size_t *num_values, int channels, int sample_rate,
                                             float hash_duration, bool persist);
/* The same with the samples in `format` (enum NeedleHipSampleFormat; planar: analyzer videos * channels pointers): they
 * are uploaded as they are and converted on the device, group by group under the uploads, in front of the down-mix
 * (fused into the conversion), the resampler and the fingerprinter.  With NEEDLE_HIP_SAMPLE_S16 this is
 * needle_hip_analyzer_run_pcm. */
enum NeedleError needle_hip_analyzer_run_pcm_format(struct NeedleAudioAnalyzer *analyzer, const void *const *pcm,
                                                    const size_t *num_values, int channels, int sample_rate, int format,
                                                    float hash_duration, bool persist);

/* ---- Comparator in memory ------------------------------------------------------------------------- */
typedef struct NeedleHipSearchResult {
  bool has_result; /* false: the reference pushes no SearchResult for this video (comparator.rs:608-617) */
  bool has_opening;
  bool has_ending;
  uint64_t opening_start_ns, opening_end_ns;
  uint64_t ending_start_ns, ending_end_ns;
} NeedleHipSearchResult;

/* Comparator::run_with_frame_hashes (comparator.rs:524-629).  `results` has one slot per video. */
enum NeedleError needle_hip_comparator_run_with_frame_hashes(const struct NeedleAudioComparator *comparator,
                                                             const FrameHashes *const *frame_hashes,
                                                             size_t num_videos, bool display,
                                                             bool use_skip_files, bool write_skip_files,
                                                             NeedleHipSearchResult *results);

/* The host half of that call on its own: the order-sensitive epilogue (reverse-walk order, duration validity,
 * BinaryHeap array order, find_best_match; comparator.rs:191-249,405-515,583-626) from a COMPLETE run list of all
 * pairs (NeedleHipRun.problem = pair index * regions + region, regions = 2 with endings) to the results of videos
 * [first_video, first_video + video_count); the other slots are left empty.  No device work: this is what every rank
 * of a multi-GPU job runs for its own block of videos after the run lists have been all-gathered. */
enum NeedleError needle_hip_comparator_results_from_runs(const struct NeedleAudioComparator *comparator,
                                                         const FrameHashes *const *frame_hashes, size_t num_videos,
                                                         const NeedleHipRun *runs, size_t num_runs, size_t first_video,
                                                         size_t video_count, NeedleHipSearchResult *results);

/* ---- Match evidence: why a video got its result ------------------------------------------------------
 * One record per region of a video: the candidate find_best_match picked (comparator.rs:405-515; ascending (-score,
 * candidate index), first), the pair it came from and how many of the video's candidates agree with it.  For a region
 * that has a match, result.start == start_ns + time_padding and result.end == end_ns - time_padding - the video's hash
 * duration.  A video without a result, a region without a match and, without include_endings, every `ending` read
 * partner = UINT32_MAX and every other field 0. */
typedef struct NeedleHipMatchEvidence {
  uint32_t partner;      /* position of the OTHER video of the winner's pair; UINT32_MAX: this region has no match, every other field 0 */
  uint32_t is_source;    /* 1: this video is that pair's source (the lower position) */
  uint32_t candidate;    /* the winner's index in the video's candidate list (comparator.rs:410-432 order) */
  uint32_t candidates;   /* length of that list (openings and endings together, as the reference builds it) */
  uint32_t support;      /* `count` of :466 for the winner: candidates with popcount(hash ^ winner.hash) < threshold + threshold / 2, the winner included, both regions (:436-453) */
  uint32_t partners;     /* distinct partner videos among those `support` candidates */
  float    score;        /* count * 0.3f + secs * 0.7f in f32, two roundings, no fused multiply-add: the negated key of :469 */
  uint32_t match_hash, partner_hash;       /* the winner's simhash on this video's side / on the partner's */
  uint32_t reserved;                       /* 0 */
  uint64_t start_ns, end_ns;               /* the winner's interval in THIS video before padding (:476) */
  uint64_t partner_start_ns, partner_end_ns; /* the same run's interval in the partner */
} NeedleHipMatchEvidence;
typedef struct NeedleHipSearchEvidence { NeedleHipMatchEvidence opening, ending; } NeedleHipSearchEvidence;

/* needle_hip_comparator_results_from_runs with the evidence beside the results: the same arguments, checks and failures,
 * no device work.  `evidence` has one slot per video, as `results` (the slots outside [first_video, first_video +
 * video_count) read "no match"); `results` may be NULL.  What it writes to `results` is what the call above writes. */
enum NeedleError needle_hip_comparator_results_from_runs_evidence(const struct NeedleAudioComparator *comparator,
                                                                  const FrameHashes *const *frame_hashes, size_t num_videos,
                                                                  const NeedleHipRun *runs, size_t num_runs, size_t first_video,
                                                                  size_t video_count, NeedleHipSearchResult *results,
                                                                  NeedleHipSearchEvidence *evidence);

/* ---- A library of many shows: groups of videos ---------------------------------------------------------
 * `groups` gives every video a label (any 32-bit value); videos of equal label are one season, and only pairs INSIDE a
 * season are searched: no scan, no candidate and no result ever crosses a season.  A video's result -- and with `display`
 * and the skip-file switches what is printed for it and what its skip file holds -- is what the ungrouped call over its own
 * season's videos, in list order, gives it; the videos are walked in list order, and where several fail the call fails
 * with the one at the lowest position.  A video alone in its season has no pair and no result.
 *
 * The grouped pair numbering: seasons are numbered in the order their first video appears, a season's members are its
 * list positions in ascending order (they need not be adjacent), n_g of them; base_g = sum over h < g of
 * n_h (n_h - 1) / 2, and pair (a, b), a < b, of season g with ranks (ra, rb) among its members is base_g +
 * ra (2 n_g - ra - 1) / 2 + (rb - ra - 1): the i-major order inside the season, and with one season the ungrouped
 * numbering.  NeedleHipRun.problem = NeedleHipProblem.tag = grouped pair id * regions + region.
 *
 * needle_hip_group_pairs: the number of grouped pairs into *num_pairs and, where pair_videos is not NULL, the (a, b) of
 * pairs 0 .. min(capacity, *num_pairs) - 1 as pair_videos[2 p], pair_videos[2 p + 1]: to size buffers and decode `problem`. */
enum NeedleError needle_hip_group_pairs(const uint32_t *groups, size_t num_videos, uint32_t *pair_videos, size_t capacity,
                                        uint64_t *num_pairs);
/* needle_hip_comparator_run_with_frame_hashes over the seasons of `groups` (num_videos labels); groups == NULL is that
 * call.  NeedleError_InvalidArgument where grouped pairs x regions, or the hashes, exceed 2^32.  With endings, "no ending
 * hash data present" only concerns videos that have a pair.  The library job takes groups through
 * needle_hip_library_set_groups, the index and the cross-matcher through their own calls (further down); match evidence
 * and NeedleHipMatcher do not take groups. */
enum NeedleError needle_hip_comparator_run_with_frame_hashes_grouped(const struct NeedleAudioComparator *comparator,
                                                                     const FrameHashes *const *frame_hashes, size_t num_videos,
                                                                     const uint32_t *groups, bool display, bool use_skip_files,
                                                                     bool write_skip_files, NeedleHipSearchResult *results);
/* The host half of the grouped call on its own, no device work: from a COMPLETE grouped run list (problem = grouped pair
 * id * regions + region) to the results of all videos.  NeedleError_InvalidArgument for a run whose problem is beyond the
 * grouped pairs x regions (a list in another numbering).  groups == NULL: needle_hip_comparator_results_from_runs over
 * all videos. */
enum NeedleError needle_hip_comparator_results_from_runs_grouped(const struct NeedleAudioComparator *comparator,
                                                                 const FrameHashes *const *frame_hashes, size_t num_videos,
                                                                 const uint32_t *groups, const NeedleHipRun *runs, size_t num_runs,
                                                                 NeedleHipSearchResult *results);
/* needle_audio_comparator_run (the file-based call: hashes from the .needle.dat files, or analyzed first) over the seasons
 * of `groups`, parallel to the comparator's paths: num_groups_entries must be their number (InvalidArgument otherwise).
 * groups == NULL: the ungrouped call. */
enum NeedleError needle_hip_comparator_run_grouped(const struct NeedleAudioComparator *comparator, const uint32_t *groups,
                                                   size_t num_groups_entries, bool analyze, bool display, bool use_skip_files,
                                                   bool write_skip_files);

/* ---- Incremental index: a growing library searched one append at a time ---------------------------------
 * Results equal needle_hip_comparator_run_with_frame_hashes over ALL videos added so far, in insertion order, bit for
 * bit; an append searches only the pairs it adds (old x new and new x new) and recomputes the best match only of the
 * videos whose candidate list changed.  The index copies the comparator's parameters (threshold, minimum durations,
 * padding, include_endings) at creation: later changes to the comparator do not affect it.  The videos' hashes are
 * copied; the caller may free its FrameHashes after an add.  One GPU: the index runs on the device that was current when
 * it was created (no sharding across ranks).  Videos can be removed or replaced in place; no display or skip files. */
typedef struct NeedleHipIndex NeedleHipIndex;
enum NeedleError needle_hip_index_new(const struct NeedleAudioComparator *comparator, NeedleHipIndex **output);
void needle_hip_index_free(NeedleHipIndex *index);
size_t needle_hip_index_len(const NeedleHipIndex *index); /* videos added (0 for NULL) */
/* Appends k >= 1 videos.  Fails as run_with_frame_hashes would over the longer list (no ending data with endings on,
 * padding or hash duration beyond a match's end, more than 2^32 hashes or sequence pairs: NeedleError_InvalidArgument);
 * after a failure the index is exactly as it was before the call. */
enum NeedleError needle_hip_index_add(NeedleHipIndex *index, const FrameHashes *const *frame_hashes, size_t k);
/* One result per video added, in insertion order; n >= needle_hip_index_len(index) (NeedleError_InvalidArgument otherwise). */
enum NeedleError needle_hip_index_results(const NeedleHipIndex *index, NeedleHipSearchResult *results, size_t n);
/* One evidence record per video, in insertion order, for the results above (n as there).  Computed on the device from the
 * committed store when the call is made: `partner` is a current position, whatever was removed or replaced before, and
 * nothing is kept between calls.  The index is not changed.  One wait. */
enum NeedleError needle_hip_index_evidence(const NeedleHipIndex *index, NeedleHipSearchEvidence *evidence, size_t n);
/* Video pairs that entered the index: over its life (*total) and by the last successful add (*last).  A pair none
 * of whose sequences can hold a run long enough is left out, as in the full search.  Either pointer may be NULL.
 * (needle_hip_index_pairs_scanned: those of them the one-shot scan searched.) */
enum NeedleError needle_hip_index_pairs_searched(const NeedleHipIndex *index, uint64_t *total, uint64_t *last);
/* Removes the videos at k >= 1 distinct positions (< needle_hip_index_len).  The others keep their relative order.  Results
 * then equal run_with_frame_hashes over the remaining list.  No pair is scanned (pairs_searched: *last = 0, total unchanged).
 * Fails like a full search of that list would (padding / hash duration beyond the new winner's match end).  After any
 * failure the index is exactly as it was.  NULL pointers: NeedleError_NullArgument; k == 0, a position out of range or
 * repeated: NeedleError_InvalidArgument. */
enum NeedleError needle_hip_index_remove(NeedleHipIndex *index, const size_t *positions, size_t k);
/* Replaces the videos at k >= 1 distinct positions with frame_hashes[0..k), in place (positions[i] gets frame_hashes[i]).
 * Only the pairs that involve a replaced video are scanned (*last = their number, total += it).  Otherwise it behaves like
 * needle_hip_index_add (and fails like remove on bad positions). */
enum NeedleError needle_hip_index_replace(NeedleHipIndex *index, const size_t *positions, const FrameHashes *const *frame_hashes,
                                          size_t k);
/* sizes[0] heap entries held (sum of the buckets' valid counts), sizes[1] entry slots in use, sizes[2] hashes in the
 * device arena, sizes[3] timestamps in the device table.  After a remove or replace sizes[0] == sizes[1]. */
enum NeedleError needle_hip_index_store_sizes(const NeedleHipIndex *index, uint64_t sizes[4]);

/* ---- A grouped index: a library of many shows that grows in place ---------------------------------------------
 * The incremental index over groups of videos (above, "A library of many shows").  A grouped index is made as such; every
 * video is added with a label (any values: they are only compared, equal labels are one season) and only pairs inside a
 * season are searched.  Results equal needle_hip_comparator_run_with_frame_hashes over each season's own sub-list of the
 * current list, bit for bit -- what needle_hip_comparator_run_with_frame_hashes_grouped gives over the current list -- and a
 * video alone in its season has no result.  An append searches only the arriving videos' pairs with the members of their
 * seasons before them in the list (pairs_searched and pairs_scanned count those), whatever the size of the library; every
 * other season's results and stored entries stay where they are.
 * needle_hip_index_results, _evidence (`partner` is a current position of the same season), _remove, _replace (the new video
 * keeps the label of the position it replaces; only its season's pairs are scanned), _pairs_searched, _pairs_scanned,
 * _store_sizes and _len work on a grouped index as on a plain one.  "no ending hash data present" concerns only a video that
 * has a pair.  Refused with NeedleError_InvalidArgument, before any device work: needle_hip_index_add on a grouped index,
 * needle_hip_index_add_grouped on a plain one, and needle_hip_index_crossmatcher_new, _matcher_new, _add_matched and
 * _add_streamed on a grouped one.  A season streamed into a grouped index goes through
 * needle_hip_index_crossmatcher_new_grouped / needle_hip_index_add_matched_grouped (further down). */
enum NeedleError needle_hip_index_new_grouped(const struct NeedleAudioComparator *comparator, NeedleHipIndex **output);
/* Appends k >= 1 videos, groups[i] the label of frame_hashes[i].  Otherwise as needle_hip_index_add. */
enum NeedleError needle_hip_index_add_grouped(NeedleHipIndex *index, const FrameHashes *const *frame_hashes, const uint32_t *groups,
                                              size_t k);
/* The current list's labels, one per video; n >= needle_hip_index_len(index).  A plain index: NeedleError_InvalidArgument. */
enum NeedleError needle_hip_index_groups(const NeedleHipIndex *index, uint32_t *labels, size_t n);

/* ---- Library: an HBM-resident analyze+search job, shardable across GPUs ----------------------------
 * One object per process/GPU describing ALL videos of a job.  PCM of the videos this rank owns is
 * uploaded once and stays in HBM; hashes live in a padded device arena [video * rows_per_video][stride] so a
 * plain all-gather over contiguous video blocks fills the rows other ranks computed; pairs are
 * addressed by their index in the reference's lexicographic pair list (comparator.rs:534-545) -- or, in a library with
 * groups of videos (needle_hip_library_set_groups), by their grouped pair id ("A library of many shows" above): only pairs
 * inside a group exist, and every pair range, pair count and NeedleHipRun.problem of this section is in that numbering. */
typedef struct NeedleHipLibrary NeedleHipLibrary;

enum NeedleError needle_hip_library_new(size_t num_videos, float opening_search_percentage, float hash_duration,
                                        NeedleHipLibrary **output);
void needle_hip_library_free(NeedleHipLibrary *library);
/* Analyzer::with_include_endings + with_ending_search_percentage (analyzer.rs:130-139): also fingerprint the
 * last `ending_search_percentage` of every video.  Call before set_pcm; the arena then has two rows per video. */
enum NeedleError needle_hip_library_include_endings(NeedleHipLibrary *library, float ending_search_percentage);
/* The sample rate of the PCM that set_pcm, set_pcm_device, stream_pcm and rank_videos will be given (2000..768000 Hz,
 * default 11025).  Call after library_new and before set_pcm (InvalidArgument afterwards, the library unchanged).  The
 * search windows are cut at that rate, as needle_hip_analyzer_run_pcm does, and resampled to 11025 Hz mono on the device
 * on the way in: the resident PCM, and so every job's cost, is that of a mono 11025 Hz library.  The hashes equal
 * needle_hip_analyzer_run_pcm's at that rate.  At 11025 nothing is resampled.  A rate the resampler refuses (see
 * needle_hip_resample_plan) is NeedleError_InvalidArgument here, the library unchanged. */
enum NeedleError needle_hip_library_set_sample_rate(NeedleHipLibrary *library, int sample_rate);
/* A library of many shows: groups[v] is the label of video v (any 32-bit value, only compared); videos of equal label are
 * one season and only pairs INSIDE a season are searched.  Call after library_new and before set_pcm / set_pcm_device /
 * stream_pcm (InvalidArgument afterwards, and for a num_videos other than the library's; the library unchanged).  Every
 * rank passes the same labels.  On a grouped library needle_hip_library_num_pairs is the grouped pair count (what
 * needle_hip_group_pairs gives), needle_hip_library_search takes a range of grouped pair ids and writes
 * NeedleHipRun.problem = grouped pair id * comparator regions + region (what
 * needle_hip_comparator_results_from_runs_grouped takes), and finalize, job_begin / job_end and job_runs work over that
 * numbering: a video's result is what the ungrouped job over its own season's videos, in list order, gives it; a video
 * alone in its season has no result, and "no ending hash data present" concerns only a video that has a pair.  The size
 * limit of set_pcm (2^32 sequence pairs) counts grouped pairs.  One label for all videos is the plain library, run for run
 * and id for id.  A labelling without any pair is allowed: jobs succeed, every result is empty, *num_runs is 0 and nothing
 * is scanned.  rank_videos, analyze, audit, frame_hashes and the staging of PCM do not depend on the labels.
 * needle_hip_library_groups copies the labels out (n >= the library's videos); a plain library: InvalidArgument. */
enum NeedleError needle_hip_library_set_groups(NeedleHipLibrary *library, const uint32_t *groups, size_t num_videos);
enum NeedleError needle_hip_library_groups(const NeedleHipLibrary *library, uint32_t *labels, size_t n);
/* The sample format (enum NeedleHipSampleFormat, default NEEDLE_HIP_SAMPLE_S16) of the PCM that set_pcm, set_pcm_device
 * and stream_pcm will be given.  Call after library_new and before set_pcm (InvalidArgument afterwards, the library
 * unchanged).  Those three calls then read their pointer arrays in that format -- callers cast; for a planar format the
 * array has num_videos * channels entries, all planes of a video this rank does not own NULL (a mix of NULL and
 * non-NULL planes: NullArgument) -- and convert on the device on the way in: set_pcm stages the raw windows through a
 * device buffer of at most 2 GiB, set_pcm_device converts straight out of the caller's buffers.  The resident PCM is
 * what the s16 library would hold, so jobs, audit, frame_hashes and rank_videos do not depend on the format. */
enum NeedleError needle_hip_library_set_sample_format(NeedleHipLibrary *library, int format);
size_t needle_hip_library_rows_per_video(const NeedleHipLibrary *library);
/* Lengths (values per stream, all videos) are metadata every rank holds; pcm[i] may be NULL for
 * videos this rank does not own.  Crops to the opening window and uploads.  `channels` = 1..NEEDLE_HIP_MAX_CHANNELS in
 * set_pcm, set_pcm_device and stream_pcm, num_values in interleaved values; 3-8 channel windows are down-mixed on the
 * device on the way in (set_pcm through a staging buffer of at most 2 GiB), so the resident PCM is mono.  `channels` = 0,
 * here and in needle_hip_library_rank_videos: only for a library with a format per video
 * (needle_hip_library_set_video_formats, which says what the arrays then hold). */
enum NeedleError needle_hip_library_set_pcm(NeedleHipLibrary *library, const int16_t *const *pcm,
                                            const size_t *num_values, int channels);
/* The same for PCM that is already in HBM (decoded or generated on the device): d_pcm[i] are DEVICE pointers, NULL for
 * videos this rank does not own.  The search windows are copied device to device into the library's arena (at another
 * sample rate: resampled straight out of the caller's buffers, which need only 2-byte alignment); the caller's buffers
 * are free on return. */
enum NeedleError needle_hip_library_set_pcm_device(NeedleHipLibrary *library, const int16_t *const *d_pcm,
                                                   const size_t *num_values, int channels);
/* The streaming form ("analyze streamed from host-pinned PCM", BASELINE.json configs[4]): the search windows of the
 * videos with a non-NULL pointer are copied to the device in order on an upload stream and fingerprinted group by
 * group (~32 MiB of PCM each) on the library stream as they land, straight into their arena rows; nothing of the PCM
 * stays in HBM beyond a 2 GiB staging arena, and the kernels of all but the last group run underneath the copies.
 * Pinned host memory (needle_hip_host_alloc, or anything hipHostRegister'ed) is read in place by the copy engine;
 * pageable memory goes through a ring of pinned slabs filled by host threads.  On return the caller's buffers are
 * free; the last kernels may still be running (stream order: search / job_begin may follow at once).  Replaces
 * set_pcm + analyze; job_begin then skips its analyze step. */
enum NeedleError needle_hip_library_stream_pcm(NeedleHipLibrary *library, const int16_t *const *pcm,
                                               const size_t *num_values, int channels);
/* Fingerprint videos [first, first+count) into their arena rows (GPU only, no host copy). */
enum NeedleError needle_hip_library_analyze(NeedleHipLibrary *library, size_t first, size_t count, bool sync);
/* Arena geometry: device pointer to u32[num_videos * rows_per_video][stride]. */
enum NeedleError needle_hip_library_hash_arena(NeedleHipLibrary *library, uint32_t **d_arena, size_t *stride);
/* Adopt caller-owned device memory u32[rows][stride] (rows >= num_videos * rows_per_video, stride >= the library's) as the
 * arena, e.g. a buffer a collective library allocated so rows can be all-gathered in place.  Call after
 * set_pcm and before analyze; the caller keeps the memory alive and zero-initialised. */
enum NeedleError needle_hip_library_use_hash_arena(NeedleHipLibrary *library, uint32_t *d_arena, size_t rows,
                                                   size_t stride);
/* All pairs of the videos, or the grouped pair count of a library with groups. */
size_t needle_hip_library_num_pairs(const NeedleHipLibrary *library);
/* Runs of pairs [first_pair, first_pair+num_pairs) into caller-provided device buffers
 * (NeedleHipRun.problem = global pair index * comparator regions + region; the grouped pair id in a library with groups).  The fast scan kernels stage a pair's
 * destination window in LDS: up to ~39 000 hashes (2.7 h of audio at step 1, 5.3 h at the default step 2).  Pairs
 * with a longer window are scanned from HBM by a slower kernel in the same call; nothing fails (the reference has no
 * bound). */
enum NeedleError needle_hip_library_search(NeedleHipLibrary *library, const struct NeedleAudioComparator *comparator,
                                           size_t first_pair, size_t num_pairs, NeedleHipRun *d_runs,
                                           uint32_t capacity, uint32_t *d_count, bool sync);
/* Asynchronous download of a run list for pipelining jobs: _begin enqueues (on the library stream, behind the
 * search that fills them) the copy of *d_count and of the first max_runs runs into pinned host memory of
 * `slot` (0 or 1) and returns at once; _end waits for that copy only and hands back a pointer into the pinned
 * buffer (valid until the slot's next _begin).  *num_runs is the TOTAL found: if it exceeds max_runs the list
 * is truncated and the caller must fetch it synchronously.  Lets the host epilogue of job k overlap the
 * kernels of job k+1. */
enum NeedleError needle_hip_library_fetch_runs_begin(NeedleHipLibrary *library, int slot, const NeedleHipRun *d_runs,
                                                     const uint32_t *d_count, uint32_t max_runs);
enum NeedleError needle_hip_library_fetch_runs_end(NeedleHipLibrary *library, int slot, const NeedleHipRun **runs,
                                                   uint32_t *num_runs);
/* Host epilogue over the complete run list (all pairs): D2H of the arena, duration validity,
 * simhash32, BinaryHeap order, find_best_match.  `runs` is a host array. */
enum NeedleError needle_hip_library_finalize(NeedleHipLibrary *library, const struct NeedleAudioComparator *comparator,
                                             const NeedleHipRun *runs, size_t num_runs,
                                             NeedleHipSearchResult *results);
/* needle_hip_fingerprint_audit_device over the hashes this rank's share of the fingerprinting produced (all of them
 * without a communicator): the library's resident PCM through both transforms, compared with the arena's rows.  Call after
 * a job (or needle_hip_library_analyze) has filled the arena; needs set_pcm / set_pcm_device (resident PCM). */
enum NeedleError needle_hip_library_audit(NeedleHipLibrary *library, NeedleHipCertAudit *audit);
/* Copies one video's FrameHashes out of the library after analyze (+gather). */
enum NeedleError needle_hip_library_frame_hashes(NeedleHipLibrary *library, size_t index, FrameHashes **output);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI --------------------------------------------------
 * The reference parallelises inside one process with rayon when `threading` is set: over videos in
 * Analyzer::run (analyzer.rs:437-445) and over pairs in Comparator::run_with_frame_hashes
 * (comparator.rs:549-564).  Across the GPUs of a node the same two fan-outs are: the hashes of all videos in equal
 * contiguous blocks per rank, pairs in contiguous ranges of the lexicographic pair list per rank, and two all-gathers between
 * them (hash rows after analyze, run lists after search) -- all inside this library, on its own streams, with
 * librccl loaded on demand (no link-time dependency; no torch).  A process is one rank and drives one device:
 *
 *   rank 0: needle_hip_comm_create_id(id); hand the 128 bytes to the other ranks by any means (file, socket, MPI)
 *   all   : needle_hip_set_device(local_rank); needle_hip_comm_init(id, rank, world_size);
 *           library_new / set_pcm (PCM pointers for the videos of needle_hip_library_rank_videos(...) only, NULL
 *           for the rest) / job_begin / job_end ...; needle_hip_comm_finalize()
 *
 * Results are identical for every world size: the run set is a union over disjoint pair ranges and the epilogue
 * orders it.  NEEDLE_HIP_COMM=host selects a host-staged transport over POSIX shared memory instead of RCCL (ranks of
 * one node, any device assignment, e.g. two ranks on one GPU) -- for exercising the N-rank path where RCCL cannot run
 * and as a fallback; it moves data only and is not a compute fallback. */
#define NEEDLE_HIP_COMM_ID_BYTES 128
enum NeedleError needle_hip_comm_create_id(uint8_t id[NEEDLE_HIP_COMM_ID_BYTES]);
enum NeedleError needle_hip_comm_init(const uint8_t id[NEEDLE_HIP_COMM_ID_BYTES], int rank, int world_size); /* collective */
void needle_hip_comm_finalize(void);
int needle_hip_comm_rank(void);             /* 0 without a communicator */
int needle_hip_comm_world_size(void);       /* 1 without a communicator */
const char *needle_hip_comm_backend(void);  /* "none", "rccl", "host" */
enum NeedleError needle_hip_comm_barrier(void);
/* Host buffers: rank r's `bytes_per_rank` bytes land at recv + r * bytes_per_rank on every rank. */
enum NeedleError needle_hip_comm_all_gather_host(const void *send, void *recv, size_t bytes_per_rank);
/* The sharding plan: `units` (videos, pairs) in world_size contiguous blocks of ceil(units / world_size). */
void needle_hip_comm_shard(size_t units, int world_size, int rank, size_t *first, size_t *count);

/* Which videos' PCM a rank has to hold.  The fingerprinting is sharded by HASHES, not by videos: the arena
 * u32[rows][stride] is cut, as one flat array, into world_size equal blocks and a rank computes the hashes of its block
 * from the stretch of PCM they depend on -- 28 episodes on 8 ranks are 3.5 episodes' worth of frames each, no rank
 * idles (whole videos would give 7 x 4 + 0).  For the stream lengths `num_values` (all videos; what set_pcm will be
 * given) this names the videos [first_video, first_video + video_count) whose rows rank `rank`'s block meets: pass
 * their PCM to set_pcm, NULL for the others.  A pure function of the library's parameters and the lengths. */
enum NeedleError needle_hip_library_rank_videos(const NeedleHipLibrary *library, const size_t *num_values, int channels,
                                                int world_size, int rank, size_t *first_video, size_t *video_count);

/* One analyze+search job of the library across the communicator (or on one GPU without one), in two halves so
 * that two jobs can be in flight (slot 0 / 1): _begin enqueues this rank's fingerprinting, the all-gather of hash
 * rows, the scan of this rank's pair range, the all-gather of run lists and their download, and returns at once;
 * _end waits for that download, runs the per-video epilogue (find_best_match, comparator.rs:583-626; sharded by video
 * across ranks with one more all-gather once it is large enough to pay for it) and fills results[num_videos] on
 * every rank.  *num_runs (optional): runs found over all pairs. */
enum NeedleError needle_hip_library_job_begin(NeedleHipLibrary *library, const struct NeedleAudioComparator *comparator,
                                              int slot);
enum NeedleError needle_hip_library_job_end(NeedleHipLibrary *library, const struct NeedleAudioComparator *comparator,
                                            int slot, NeedleHipSearchResult *results, size_t *num_runs);
/* The complete run list (all pairs, all ranks' shares in rank order) the epilogue of the job that finished last in
 * `slot` worked from: host memory of the library, valid until the slot's next job_begin.  For checkers and callers
 * that want the segments themselves ("the final cross-shard pair list"), not only the per-video results.
 * With more than one rank and the sharded device epilogue (library scale) the runs travel OWNER-DIRECTED from the
 * library's third job on -- a run of pair (i, j) to the ranks that own videos i and j (the epilogue of a video needs its
 * own pairs and nothing else, comparator.rs:583-588), sizes from the previous job's count matrix -- and a rank then holds,
 * and this call returns (downloaded on demand), the runs of ITS videos' pairs only; *num_runs of job_end stays the
 * total over all ranks.  NEEDLE_HIP_DIRECTED_RUNS=0: every job gathers every rank's runs on every rank, as before. */
enum NeedleError needle_hip_library_job_runs(const NeedleHipLibrary *library, int slot, const NeedleHipRun **runs,
                                             size_t *num_runs);
/* What the collectives of that job moved, as received per rank: bytes[0] hash rows (all-gather of the arena's blocks),
 * bytes[1] run lists (the gathered heads, or the owner-directed blocks + the count matrix; repeats included), bytes[2] per-video results of a sharded
 * epilogue; bytes[3] = scans repeated because a slab or a head overflowed (0 in the steady state). */
enum NeedleError needle_hip_library_job_comm_bytes(const NeedleHipLibrary *library, int slot, uint64_t bytes[4]);
/* Which forms the job that finished last in `slot` took: form[0] 1 = per-video epilogue on the device (0: host threads;
 * a device epilogue handed back to the host counts in needle_hip_epilogue_host_fallbacks), form[1] 1 = epilogue sharded by
 * video across ranks, form[2] 1 = runs exchanged owner-directed, form[3] the scan's form (needle_hip_scan_last_launch).
 * The epilogue goes to the device from 16 384 sequence pairs -- or, whatever the pair count, once the library's last
 * finished job found 16 384 runs or more per rank (stretches of silence, sustained chords: the run list, not the pair
 * count, is what the host form pays for; NEEDLE_HIP_DEVICE_EPILOGUE=0 / 1 forces either). */
enum NeedleError needle_hip_library_job_form(const NeedleHipLibrary *library, int slot, uint32_t form[4]);
/* Host threads this process uses for its parallel host phases (epilogue, file reads, upload staging): the CPUs usable
 * by the process (affinity, cgroup quota) divided by the rank processes of the node once a communicator is up
 * (LOCAL_WORLD_SIZE if the launcher exports it, else the world size); NEEDLE_HOST_THREADS overrides. */
int needle_hip_host_threads(void);

/* ---- Streaming fingerprinter: chromaprint's start / feed / finish, batched over lanes -------------------
 * N lanes, one per decoder.  A feed takes whatever every lane has decoded since the last one; the per-lane state (the
 * PCM tail from the first frame of the first item not yet emitted, and the first pass's chroma / energy rows of its
 * frames: at most 76 KB per mono lane) stays in device memory and does not grow with the stream.  Every frame goes
 * through the first pass once.  After `finish` a lane's items are bit for bit those of needle_hip_fingerprint_host (or
 * of needle_hip_analyzer_run_pcm_format's opening hashes with the window set to the whole stream) over the
 * concatenation of its chunks, however they were cut, also under NEEDLE_HIP_STFT=f64; items reported earlier are a
 * prefix of that sequence and are never revised.
 *
 * channels 1..8, sample_rate 2000..768000 and every NeedleHipSampleFormat: what needle_hip_analyzer_run_pcm_format
 * takes, through the same path -- conversion, the fused down-mix of 3-8 channels, the resampler, the fingerprinter.  At
 * another rate than 11025 Hz a lane also keeps the source samples the resampler's next output tile still reads.
 *
 * A chunk is whole frames (num_values[i] % channels != 0: InvalidArgument, checked for every lane before any device
 * work); a non-empty chunk for a finished lane is InvalidArgument until `reset`.  On return from `feed` the caller's
 * buffers may be reused.  A feed of more than NEEDLE_HIP_MAX_BATCH_VALUES values (default 2^30) is cut internally.
 * `ready` and `items` wait for outstanding device work.  A device failure poisons the feeder: every later call returns
 * it.  One thread at a time per feeder.
 *
 * needle_hip_feeder_ready's kept_items is a function of the samples fed and of `finished` alone, not of how they were
 * cut: it equals needle_hip_feeder_num_ready(...).  Finished that is num_kept(resample_out_len(n, rate), step).
 * Unfinished, a feed resamples the whole output tiles whose taps lie inside the samples fed (the stream's end is not
 * known, nothing may be clamped) and the first pass has seen the whole frame PAIRS of those outputs (the two-for-one
 * transform pairs frames (2p, 2p + 1); a trailing odd frame waits for its partner).  The count therefore lags the
 * one-shot's on the same prefix by at most L raw items -- ceil(L / step) kept items -- where, with T the resampler's
 * tile and h its filter's half length in outputs, L = ceil((T + h) / 1365) + 1:
 *     11025 Hz (no resampler)                          L = 1
 *     44100 Hz (integer decimation, T = 1280)          L = 2
 *     22050 Hz (integer decimation, T = 1536)          L = 3
 *     48000 / 96000 Hz (matrix cores / DPP, T = 2352)  L = 3
 *     32000 Hz (matrix cores, T = 7056)                L = 7
 *     12345 Hz (a rate coprime-ish to 11025: the general form, T = 11760)   L = 10
 * (T = 16 x 11025 / gcd(11025, rate) outside the integer decimations: a rate that shares little with 11025 has long
 * tiles, and its items arrive in steps of that many outputs.) */
typedef struct NeedleHipFeeder NeedleHipFeeder;
enum NeedleError needle_hip_feeder_new(size_t lanes, int channels, int sample_rate, int format, uint32_t step,
                                       NeedleHipFeeder **output);
void needle_hip_feeder_free(NeedleHipFeeder *feeder);
/* one entry per lane (planar formats: lanes * channels pointers, as in run_pcm_format); num_values[i] == 0: nothing for lane i */
enum NeedleError needle_hip_feeder_feed(NeedleHipFeeder *feeder, const void *const *pcm, const size_t *num_values);
enum NeedleError needle_hip_feeder_finish(NeedleHipFeeder *feeder, const size_t *lanes, size_t k); /* NULL: every unfinished lane */
enum NeedleError needle_hip_feeder_reset(NeedleHipFeeder *feeder, const size_t *lanes, size_t k);  /* lane starts a new stream; NULL: every lane */
enum NeedleError needle_hip_feeder_ready(NeedleHipFeeder *feeder, size_t lane, size_t *kept_items,
                                         uint64_t *samples_per_channel_fed, bool *finished);
enum NeedleError needle_hip_feeder_items(NeedleHipFeeder *feeder, size_t lane, size_t first, size_t count, uint32_t *items);
/* FrameHashes of one video from two finished lanes: attach_timestamps (analyzer.rs:293-318) with ending_seek_ns as the
 * ending window's seek offset (:314-318).  Requires step == the step of hash_duration.  ending_lane SIZE_MAX: no ending. */
enum NeedleError needle_hip_feeder_frame_hashes(NeedleHipFeeder *feeder, size_t opening_lane, size_t ending_lane,
                                                uint64_t ending_seek_ns, float hash_duration, const char *md5, FrameHashes **output);
/* bytes[0]: the most state any one lane has carried from one round to the next so far, as the carry moved it (PCM
 * tail, source-rate tail and rows; 0 before the second feed).  It does not grow with the stream: at most 22 frames'
 * rows (112 B each), (24 x 1365 + 4096) samples of 11025 Hz PCM per tail channel and, at another rate, the inputs of one
 * resampler tile plus its filter's length -- 76 176 B for a mono lane at 11025 Hz, 149 888 B for stereo at 11025 Hz,
 * 117 760 B for stereo at 48 kHz.  bytes[1]: high-water of one round's staging (new samples and raw chunks). */
enum NeedleError needle_hip_feeder_state_bytes(const NeedleHipFeeder *feeder, uint64_t bytes[2]);
/* The audit of the f32 first pass (NeedleHipCertAudit above), travelling with the stream: the feeder path never holds a
 * window of PCM, so it cannot be audited from outside.  An audited round runs everything a round runs, then at most two
 * more launches -- the f64 kernel over the round's NEW frame pairs, into f64 chroma rows the audit carries beside the
 * first pass's (every pair goes through it once), and the audit kernel over carried + new -- and downloads nothing more:
 * the counts stay on the device, one set per lane, until needle_hip_feeder_audit asks.  A lane's audit covers exactly the
 * kept items its current stream has emitted so far (`items` == needle_hip_feeder_ready's kept_items after any round;
 * counts never decrease within a stream; needle_hip_feeder_reset clears the lane's), `mismatches` compares the items the
 * feeder itself emitted, K is NEEDLE_HIP_CERT_K as every feed reads it, and the six fields equal those of
 * needle_hip_library_audit / needle_hip_fingerprint_audit_device over the same stream, however it was cut.
 * A feeder that does not ask for the audit launches and keeps exactly what it did without it.
 * With the audit on, needle_hip_feeder_state_bytes' bytes[0] counts the audit's carried rows too, 96 B each:
 *     bytes[0] <= (bound without the audit) + 22 x 96 B      (78 288 B for a mono lane at 11025 Hz)
 * and a round holds, besides, 96 B per new frame of every lane.
 * set_audit: only while no lane holds samples (a new feeder, or every lane reset); otherwise InvalidArgument, nothing
 * changed.  audit: lane < lanes: that lane's current stream; lane == SIZE_MAX: all lanes (counts summed, maxima taken);
 * waits for the library stream; InvalidArgument when the audit is off.  Under NEEDLE_HIP_STFT=f64 there is no first pass
 * to audit: set_audit(true), and a feed of an audited feeder, fail with InvalidArgument before any device work. */
enum NeedleError needle_hip_feeder_set_audit(NeedleHipFeeder *feeder, bool on);
enum NeedleError needle_hip_feeder_audit(NeedleHipFeeder *feeder, size_t lane, NeedleHipCertAudit *audit);
/* pure host arithmetic, no device: kept items a lane holds after that many samples */
size_t needle_hip_feeder_num_ready(uint64_t samples_per_channel_fed, int sample_rate, int channels, uint32_t step, bool finished);

/* ---- A feeder whose lanes have a rate, a channel count and a sample format of their own -------------------
 * A season is rarely uniform (stereo 44.1 kHz episodes among 5.1 48 kHz ones, one planar-float rip): such a feeder takes
 * it whole, one lane per decoder as before, and is what the matchers' feed_from_feeder and frame_hashes want -- one
 * feeder whose lanes are the season's.  Limits per lane: those of needle_hip_feeder_new (channels 1..8, sample_rate
 * 2000..768000, every NeedleHipSampleFormat), checked for every lane before any device is asked for.
 *
 * The pointer array of `feed` is the concatenation, lane after lane, of each lane's planes: 1 pointer for an
 * interleaved lane, channels_i for a planar one.  num_values[i] counts lane i's values (frames x channels_i); a chunk
 * that is not whole frames of its own lane is InvalidArgument before any device work.  finish, reset, ready, items,
 * frame_hashes, state_bytes, set_audit, audit and both feed_from_feeder mean what they mean above; ready's kept_items
 * equals needle_hip_feeder_num_ready(samples, rate_i, channels_i, step, finished) with the lane's own rate.
 *
 * Every lane of such a feeder is reduced to MONO as it lands -- needle_hip_convert_host's conversion, then
 * needle_hip_downmix_host's (sum of the frame) / channels, 2 channels included -- by one kernel launch per round whatever
 * the mixture, so both tails of every lane are mono: state_bytes' bytes[0] stays within the mono bound of the lane's
 * rate (76 176 B at 11025 Hz) whatever the channel count.  The items are those of the one-shot path all the same: every
 * reader of stereo PCM there (the transform at 11025 Hz, the resampler elsewhere) begins with the same integer
 * (L + R) / 2, C truncation.  Behind the landing a round is the round of needle_hip_feeder_new's feeder, the resampler
 * launched once per distinct rate other than 11025 Hz among the lanes that complete output tiles in it.
 *
 * A feeder made by needle_hip_feeder_new is untouched by all this: its launches, its state (stereo tails stay stereo),
 * its state_bytes; it refuses reset_format (InvalidArgument, nothing changed).  lane_format works on both kinds. */
typedef struct NeedleHipLaneFormat {
  int32_t channels;
  int32_t sample_rate;
  int32_t format; /* enum NeedleHipSampleFormat */
} NeedleHipLaneFormat;
enum NeedleError needle_hip_feeder_new_lanes(const NeedleHipLaneFormat *formats, size_t lanes, uint32_t step, NeedleHipFeeder **output);
enum NeedleError needle_hip_feeder_lane_format(const NeedleHipFeeder *feeder, size_t lane, NeedleHipLaneFormat *format);
/* lanes[j] starts a new stream in formats[j] (as needle_hip_feeder_reset, which keeps a lane's format); only on a feeder
 * made by needle_hip_feeder_new_lanes.  Every lane and every format -- its limits, and that the resampler has a design for
 * its rate (a few rates inside the limits have none: 11025 / 44101 is too long a ratio, as for needle_hip_feeder_new) -- is
 * checked before any lane is reset: InvalidArgument, nothing changed, not for the lanes named earlier in the call either. */
enum NeedleError needle_hip_feeder_reset_format(NeedleHipFeeder *feeder, const size_t *lanes, const NeedleHipLaneFormat *formats, size_t k);
/* The front end of such a feeder on its own: out[i] receives mono s16, num_values[i] / channels_i values (a trailing
 * partial frame is dropped); pcm is the concatenation of the streams' planes as in `feed`; sample_rate is not looked at.
 * One kernel launch per batch of at most NEEDLE_HIP_MAX_BATCH_VALUES values, whatever the mixture of formats. */
enum NeedleError needle_hip_convert_mono_host(const void *const *pcm, const size_t *num_values, const NeedleHipLaneFormat *formats,
                                              size_t num_streams, int16_t *const *out);

/* ---- Channel mixes: a layout-aware fold-down to stereo, then mono, on the device ---------------------------
 * The reference hands chromaprint stereo only (analyzer.rs:180-187,218): a 5.1 track goes through its resampler's
 * rematrix first, so a surround episode and a stereo episode of one show hash alike.  The plain average of the C
 * channels above does not give that; a channel mix does.  It is an OPTION on every path that takes C-channel PCM:
 * nothing changes for a caller who sets none.
 *
 * A mix is a 2 x C matrix of Q15 integers, coef[0][c] to the left output and coef[1][c] to the right.  For one frame of
 * C samples x_c, each converted to s16 first by the sample format's rule above:
 *   acc_o  = sum over c of coef[o][c] * x_c                       (o = 0, 1; int32)
 *   Lo, Ro = clip((acc_o + 16384) >> 15, -32768, 32767)           (arithmetic shift)
 *   mono   = (Lo + Ro) / 2                                        (C division: the stereo path's own rule)
 * Limits, each NeedleError_InvalidArgument on the host before any device is asked for: channels outside 1..8; a
 * coefficient outside [-32768, 32768]; a row whose sum of |coef| exceeds 65535 (the bound that keeps acc in int32); and
 * channels different from the channel count of the call, the library or the lane the mix is given to.
 * The arithmetic is this front end's own specification.  The default weights are shaped after swresample's documented
 * defaults as recalled; swresample itself could not be compared against. */
typedef struct NeedleHipChannelMix {
  int32_t channels;
  int32_t coef[2][NEEDLE_HIP_MAX_CHANNELS];
} NeedleHipChannelMix;
/* The default mix of a channel mask (WAVEFORMATEXTENSIBLE / FFmpeg bits: 0x1 FL, 0x2 FR, 0x4 FC, 0x8 LFE, 0x10 BL,
 * 0x20 BR, 0x40 FLC, 0x80 FRC, 0x100 BC, 0x200 SL, 0x400 SR; channels in ascending bit order).  Weights: FL, FLC 1 to
 * the left; FR, FRC 1 to the right; FC sqrt(1/2) to both; BL, SL sqrt(1/2) to the left; BR, SR sqrt(1/2) to the right;
 * BC 1/2 to both; LFE 0.  Both rows are divided by the larger row sum if that exceeds 1, then
 * coef = floor(m * 32768 + 0.5).  A bit above 0x400, or a popcount outside 1..8, is InvalidArgument.  Host arithmetic. */
enum NeedleError needle_hip_channel_mix_default(uint32_t channel_mask, NeedleHipChannelMix *out);
/* The kernel alone, like needle_hip_convert_mono_host: out[i] receives the mono of stream i under mixes[i];
 * mixes[i].channels == 0 asks for the plain average of stream i.  One launch of the rematrix kernel per batch. */
enum NeedleError needle_hip_rematrix_host(const void *const *pcm, const size_t *num_values, const NeedleHipLaneFormat *formats,
                                          const NeedleHipChannelMix *mixes, size_t num_streams, int16_t *const *out);
/* The drivers.  With a mix set, C-channel input of any format (1 and 2 channels included) is landed as mono by the
 * rematrix kernel and everything behind it is the mono s16 path on those values.
 * analyzer: for needle_hip_analyzer_run_pcm / _run_pcm_format, whose `channels` must equal the mix's.  NULL: plain again. */
enum NeedleError needle_hip_analyzer_set_channel_mix(struct NeedleAudioAnalyzer *analyzer, const NeedleHipChannelMix *mix);
/* file analyzer (needle_audio_analyzer_run): every WAVE_FORMAT_EXTENSIBLE file whose dwChannelMask is non-zero and is
 * accepted by needle_hip_channel_mix_default is folded with its own default mix; other files keep the plain average. */
enum NeedleError needle_hip_analyzer_set_layout_downmix(struct NeedleAudioAnalyzer *analyzer, bool on);
/* the same for the analyzer that needle_audio_comparator_run makes when asked to `analyze` */
enum NeedleError needle_hip_comparator_set_layout_downmix(struct NeedleAudioComparator *comparator, bool on);
/* library: before set_pcm / set_pcm_device / stream_pcm, like set_sample_format; the channel count of those calls must
 * equal the mix's.  NULL: plain again. */
enum NeedleError needle_hip_library_set_channel_mix(NeedleHipLibrary *library, const NeedleHipChannelMix *mix);
/* feeder: lanes[j] takes mixes[j] (channels == 0: none).  Only on a feeder made by needle_hip_feeder_new_lanes, and only
 * for lanes that hold no samples (new or reset); otherwise InvalidArgument and nothing changes, not for lanes named
 * earlier in the call either.  reset_format clears a lane's mix.  A feeder any of whose lanes has a mix lands every
 * staged span of a round with one launch of the rematrix kernel (timer "rematrix"; no "ingest" launch); one without
 * launches what it always did. */
enum NeedleError needle_hip_feeder_set_lane_mix(NeedleHipFeeder *feeder, const size_t *lanes, const NeedleHipChannelMix *mixes, size_t k);

/* ---- Library and analyzer: a rate, channel count, sample format and mix per video ----------------------------
 * A season is rarely uniform: stereo 44.1 kHz episodes among 5.1 48 kHz ones, one planar-float rip among s16 ones.  The
 * batch path takes such a season as it is.
 *
 * needle_hip_library_set_video_formats: formats[num_videos]; mixes NULL, or mixes[num_videos] with channels == 0
 * meaning the plain average for that video.  After needle_hip_library_new (and include_endings), before any PCM call:
 * later it is InvalidArgument.  It excludes set_sample_rate, set_sample_format and set_channel_mix: calling one of them
 * after it, or it after one of them, is InvalidArgument.  It may be called again before the PCM arrives; video_format
 * reports what was last accepted (InvalidArgument on a library without formats, or for a video out of range).
 * Limits per video are a feeder lane's: channels 1..8, sample_rate 2000..768000, every NeedleHipSampleFormat, a rate the
 * resampler has a design for, and a mix whose `channels` equals the video's.  Every video is checked before anything
 * changes, on the host, before a device is asked for; a refused call leaves the library exactly as it was.
 *
 * With formats set, set_pcm, set_pcm_device, stream_pcm and rank_videos are called with channels == 0 (any other value:
 * InvalidArgument; channels == 0 without formats stays InvalidArgument).  The pointer array is the concatenation, video
 * after video, of each video's planes, as in needle_hip_feeder_feed: an interleaved video gives 1 pointer, a planar one
 * channels_v pointers.  A video this rank does not hold has all its planes NULL; one with NULL and non-NULL planes is
 * NullArgument.  num_values[v] counts video v's own values (frames x channels_v).
 *
 * Each video's windows are cut at its own rate (the ending's seek included) and each window is resampled as a stream of
 * its own.  Every video lands as mono: the conversion, then the plain average (2 channels included) or the video's mix
 * -- exactly what a lane of a needle_hip_feeder_new_lanes feeder does -- so the resident PCM of such a library is
 * 11025 Hz mono s16 for every video.  Jobs, analyze, audit, frame_hashes, the arena geometry and the multi-rank
 * exchange do not depend on the formats; rank_videos(channels = 0) is a pure function of the library's parameters, the
 * formats and the lengths.  Every row of the arena is bit for bit what needle_hip_analyzer_run_pcm_format gives for that
 * video alone in its format (with the video's mix set on the analyzer, if it has one).
 *
 * Per staging batch (2 GiB, or NEEDLE_HIP_MAX_BATCH_VALUES values) set_pcm and set_pcm_device make one upload (host
 * PCM only; device PCM is read in place), ONE landing launch whatever the mixture (timer "ingest", or "rematrix" when
 * any video of the library has a mix) and one resampler launch per distinct rate other than 11025 Hz in the batch;
 * stream_pcm does the same per launch group, under the next group's uploads.  A library without formats launches
 * exactly what it always did. */
enum NeedleError needle_hip_library_set_video_formats(NeedleHipLibrary *library, const NeedleHipLaneFormat *formats,
                                                      const NeedleHipChannelMix *mixes);
enum NeedleError needle_hip_library_video_format(const NeedleHipLibrary *library, size_t video, NeedleHipLaneFormat *format);
/* needle_hip_analyzer_run_pcm_format with a format per stream: formats[num_streams]; mixes NULL, or one per stream with
 * channels == 0 for none; pcm is the concatenation of each stream's planes.  One device pass whatever the mixture; the
 * result is per video what run_pcm_format gives for it alone.  Per-stream mixes on an analyzer that has a mix of its own
 * (needle_hip_analyzer_set_channel_mix) are InvalidArgument; without them that mix is applied to every stream. */
enum NeedleError needle_hip_analyzer_run_pcm_formats(struct NeedleAudioAnalyzer *analyzer, const void *const *pcm,
                                                     const size_t *num_values, const NeedleHipLaneFormat *formats,
                                                     const NeedleHipChannelMix *mixes, float hash_duration, bool persist);

/* ---- A lane changes format in mid-stream, the fingerprint goes on ------------------------------------------
 * A decoder may report another rate, layout or sample format in the middle of a stream (a 5.1 programme among stereo
 * bumpers, a part muxed from another source); the reference then swaps its resampler and keeps feeding the SAME
 * chromaprint context (analyzer.rs:231-255, :275).  switch_format is that swap: lanes[j] ends its current SEGMENT and
 * continues its same stream in formats[j], folded by mixes[j] (mixes NULL, or mixes[j].channels == 0: the plain average;
 * the previous segment's mix ends with it).  A switch always begins a new segment, even when nothing changes.
 *
 * The lane's 11025 Hz mono signal is the concatenation of its segments, each landed and resampled as a whole stream of
 * its own: needle_hip_convert_host's rule per sample, needle_hip_downmix_host's average or needle_hip_rematrix_host's mix
 * per frame and, at any rate but 11025 Hz, needle_hip_resample_host -- ceil(n L / M) outputs for the segment's n frames,
 * the taps before its first and after its last sample zero.  The fingerprinter sees that concatenation as ONE stream:
 * frames, frame pairs, carried rows, the latency, step, certification, recomputation and the audit run across the
 * junction, and items emitted before a switch are never revised.  After `finish` the lane's items are bit for bit those
 * of needle_hip_fingerprint_host over the concatenated mono PCM, however the segments were cut into feeds, also under
 * NEEDLE_HIP_STFT=f64.  (The reference's swresample drops the old resampler's buffered tail at the swap; this front end
 * flushes it.  The difference is a fraction of a millisecond of audio and is this front end's own specification, as the
 * resampler's is.)
 *
 * Only on a feeder made by needle_hip_feeder_new_lanes (one made by needle_hip_feeder_new: InvalidArgument).  Before any
 * lane changes, every entry is checked: the lane's range, the format's limits, that the resampler has a design for the
 * rate, the mix against the new channel count, that the lane is not finished, and that no lane is named twice -- else
 * InvalidArgument and nothing has changed, not for lanes named earlier in the call either.  NULL handle, lanes or
 * formats: NullArgument.  A poisoned feeder returns its error.
 *
 * Lanes whose open segment resamples and holds samples are flushed by ONE round for all of them together, without new
 * chunks: the segment's remaining output tiles are computed with its end known, then its source tail is dropped.  The
 * lane is not finished by that: a trailing odd frame waits on for its partner, which may come from the next segment.
 * A switch of lanes at 11025 Hz, or of lanes whose open segment is empty, launches nothing and needs no device.
 *
 * Afterwards lane_format answers with the open segment's format; ready's samples_per_channel_fed is the sum of the
 * segments' frames and its kept_items equals needle_hip_feeder_num_ready_segments(lane_segments, step, finished) after
 * every call (for a lane that never switched that is needle_hip_feeder_num_ready, unchanged); state_bytes' bytes[0]
 * stays within the mono bound of the larger of the rates.  reset and reset_format clear the list of segments.  A lane
 * "holds samples" for set_audit and set_lane_mix while any segment of its current stream does: after a switch both are
 * refused as in mid-stream, although the open segment is empty (a segment's mix is given to switch_format).  A format
 * change inside one chunk is the caller's to split: switch between two feeds. */
enum NeedleError needle_hip_feeder_switch_format(NeedleHipFeeder *feeder, const size_t *lanes, const NeedleHipLaneFormat *formats,
                                                 const NeedleHipChannelMix *mixes, size_t k);
typedef struct NeedleHipSegment {
  NeedleHipLaneFormat format;
  uint64_t frames; /* samples per channel fed in that format */
} NeedleHipSegment;
/* the segments of the lane's current stream, the open one last (always at least one); *count is the number there are,
 * at most `cap` are written (out may be NULL when cap is 0) */
enum NeedleError needle_hip_feeder_lane_segments(const NeedleHipFeeder *feeder, size_t lane, NeedleHipSegment *out, size_t cap, size_t *count);
/* pure host arithmetic, no device: kept items a lane holds after these segments (the last one open unless finished).
 * 0 for no segments, step 0 or a format outside the limits (channels, sample_rate, format). */
size_t needle_hip_feeder_num_ready_segments(const NeedleHipSegment *segments, size_t count, uint32_t step, bool finished);

/* ---- Streaming comparator: search as the hashes arrive ---------------------------------------------------
 * The search half of the streaming path, the counterpart of the feeder.  A matcher holds S source sequences (the
 * openings of a season, say: the videos of an index), resident on the device from creation on, a threshold, one
 * min_len >= 1 per source, and N lanes.  A lane is a destination sequence that arrives in chunks of hashes -- from a
 * feeder lane, or from anywhere else.
 *
 * Cells, matching, runs and simhashes are those of needle_hip_hamming_runs_host above, for the problems (source s, the
 * lane's sequence, min_len[s]); NeedleHipRun.problem is the source's index.  After `finish` a lane's runs, as a set,
 * equal what that call gives for the S problems over the concatenation of the lane's chunks, both simhashes included,
 * however the chunks were cut (one-item feeds, empty feeds, a first feed of one item, which has no cell).
 *
 * When a run is reported.  After a lane has received columns [0, J) and is not finished it has reported exactly the
 * runs of the complete list with
 *     dst_end < J - 1                          (a later column has broken them), or
 *     src_end == n_s - 1 && dst_end <= J - 1   (they reached the source's last row).
 * A run that touches column J - 1 elsewhere is open; `finish` reports those of length >= min_len.  Runs are appended per
 * lane in the order they were found and never revised; the order within one feed is unspecified.
 * needle_hip_matcher_open returns (malloc'd, needle_hip_host_free) the runs still open at the last column fed whose
 * length is already >= min_len: src_end, dst_end = J - 1 and len, the simhash fields zero.  It changes nothing.
 *
 * Every cell is evaluated once: the run lengths of all diagonals at the last column fed stay in device memory between
 * feeds (one length per source row per lane, 2 bytes where every source is shorter than 65 536 hashes, else 4; two sets)
 * and a feed evaluates the cells of its new columns only, in a fixed number of kernel launches (three) that does not
 * depend on N, on S or on how many lanes have data.  A feed of more than 512 items for one lane is cut into strips of
 * 512 columns, each a round of three launches.  A lane's hashes so far are kept on the device too (4 bytes per item: the
 * destination simhash of a run reaches back into earlier chunks); the history is not bounded.
 * Nothing is lost: when a round finds more runs than its device slab holds (silence against silence makes every
 * diagonal a run) the slab grows and the round is repeated from the set of state buffers it did not write.
 * NEEDLE_HIP_MATCHER_RUN_SLAB=<runs> sets the initial slab (default 4096).
 *
 * lanes == 0 or > 65535, num_sources == 0, a min_len of 0, a source outside `hashes`, a lane out of range, items for a
 * finished lane before `reset`, unequal lane counts in feed_from_feeder: InvalidArgument, checked for every lane before
 * any device work.  The sources are uploaded at creation: without a HIP device creation fails (there is no CPU path).
 * A source shorter than 2 hashes has no cells and yields nothing.  On return from `feed` the caller's buffers may be
 * reused.  A device failure poisons the matcher: every later call returns it.  One thread at a time per matcher.
 *
 * Regions: openings against openings, endings against endings, in one object (needle_hip_matcher_new_regions).  regions is
 * 1 or 2; num_sources and lanes are multiples of it.  Source s is in region s % regions and lane l in region l % regions --
 * the numbering of the library's arena rows, of the feeder's lanes and of the cross-matcher's -- and a lane meets the
 * sources of its own region only.  NeedleHipRun.problem stays the source's index among all num_sources.  Everything above
 * holds per lane: reset, open, feed_from_feeder, the repeat after a slab overflow, strips of 512 columns; a round is still
 * three launches whatever the regions and whichever lanes have data (the grid is as wide as the larger region's sources; a
 * workgroup beyond its lane's region leaves after one table read, with no state traffic).  A lane's state holds the run
 * lengths of its own region's sources only: stats[3] = the sources + 2 sets x (lanes / regions) x the sum over the regions
 * of that region's source hashes x (2 or 4) + the histories.  Here a min_len of 0 is allowed: such a source, like one
 * shorter than 2 hashes, keeps its index but has no cells, no workgroups and no state (an index row that can hold no run
 * long enough); a lane whose region has no source with cells only counts its items.  regions == 1 with every min_len >= 1
 * is needle_hip_matcher_new, run for run.  regions 0 or > 2, num_sources or lanes not a multiple of regions:
 * InvalidArgument, before any device work; the other refusals are needle_hip_matcher_new's.
 * Out of scope: more than two regions, several ranks.  Sources taken from a device arena and runs that reach the index are
 * what needle_hip_index_matcher_new / needle_hip_index_add_streamed below do. */
typedef struct NeedleHipMatcher NeedleHipMatcher;
enum NeedleError needle_hip_matcher_new(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *sources,
                                        const uint32_t *min_len, size_t num_sources, size_t lanes, uint32_t threshold,
                                        NeedleHipMatcher **output);
/* regions 1..2; num_sources and lanes multiples of it; min_len[s] == 0: source s has no cells */
enum NeedleError needle_hip_matcher_new_regions(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *sources,
                                                const uint32_t *min_len, size_t num_sources, size_t regions, size_t lanes,
                                                uint32_t threshold, NeedleHipMatcher **output);
void needle_hip_matcher_free(NeedleHipMatcher *matcher);
/* one entry per lane, host hashes; num_items[i] == 0: nothing for lane i */
enum NeedleError needle_hip_matcher_feed(NeedleHipMatcher *matcher, const uint32_t *const *items, const size_t *num_items);
/* Moves, lane by lane (equal lane counts), the feeder's ready items the matcher has not yet taken -- those from
 * items_fed on: the lane is fed from that feeder lane alone -- and finishes the lanes the feeder has finished. */
enum NeedleError needle_hip_matcher_feed_from_feeder(NeedleHipMatcher *matcher, NeedleHipFeeder *feeder);
enum NeedleError needle_hip_matcher_finish(NeedleHipMatcher *matcher, const size_t *lanes, size_t k); /* NULL: every unfinished lane */
enum NeedleError needle_hip_matcher_reset(NeedleHipMatcher *matcher, const size_t *lanes, size_t k);  /* lane starts a new stream; NULL: every lane */
enum NeedleError needle_hip_matcher_ready(NeedleHipMatcher *matcher, size_t lane, size_t *num_runs, uint64_t *items_fed,
                                          bool *finished);
enum NeedleError needle_hip_matcher_runs(NeedleHipMatcher *matcher, size_t lane, size_t first, size_t count, NeedleHipRun *runs);
enum NeedleError needle_hip_matcher_open(NeedleHipMatcher *matcher, size_t lane, NeedleHipRun **runs, size_t *num_runs);
/* stats[0] feeds that carried items, stats[1] kernel launches, stats[2] cells evaluated (over a finished lane at most
 * (n_s - 1)(m - 1) + n_s per feed against source s; a repeated round counts again), stats[3] bytes of state on the device:
 * the sources, the two sets of run lengths and the lanes' histories (4 bytes per item fed). */
enum NeedleError needle_hip_matcher_stats(const NeedleHipMatcher *matcher, uint64_t stats[4]);

/* ---- Streaming all-pairs comparator: search a season as it is decoded ---------------------------------------
 * In a matcher every lane is a destination and every source is complete at creation.  In a cross-matcher the lanes are
 * matched AGAINST EACH OTHER: both sides of every pair grow, every cell is evaluated once, and the runs are there a
 * finish round after the last lane ends.
 *
 * The N lanes are the N videos, in order.  Pair (a, b), a < b, is the problem (src = lane a, dst = lane b, min_len): it
 * has the cells, matching, runs and simhashes of needle_hip_hamming_runs_host.  NeedleHipRun.problem is the pair's index
 * in the comparator's i-major order (the order of needle_hip_comparator_run_with_frame_hashes: (0,1), (0,2), ...,
 * (1,2), ...).  With one region, the run list therefore goes straight into needle_hip_comparator_results_from_runs; the
 * epilogue applies the duration test, so min_len is a lower bound, as in the one-shot path.  One min_len >= 1 for the
 * whole matcher: the lanes share one step, so the comparator's max(min_len[i], min_len[j]) is one number.
 *
 * When a run is reported.  Say lane a has received rows [0, Ja) and lane b columns [0, Jb).  The pair has then reported
 * exactly those runs of its final list with
 *     src_end < Ja - 1 && dst_end < Jb - 1      (an evaluated cell broke them).
 * Everything still open on the pair's frontier is reported, if its length is >= min_len, in the round in which the pair
 * becomes complete, that is when its second lane finishes.  Runs are appended to one list in the order found and never
 * revised.  The order within a round is unspecified.
 *
 * Every cell is evaluated exactly once: over finished lanes of n_a and n_b items, pair (a, b) costs (n_a - 1)(n_b - 1)
 * cells.  Between rounds a pair keeps the L-shaped frontier of its evaluated rectangle on the device (one run length per
 * row at the last column, one per column at the last row; 2 bytes where max_items < 65 536, else 4; two sets), and every
 * lane its hashes so far (the simhashes of a run reach back over earlier chunks on both sides).  A round -- a feed, a
 * piece of one (at most 512 new items per lane), or a finish -- is three kernel launches, whatever the number of lanes
 * and whichever of them have data; it uploads one lane table and the staged chunks in one copy, nothing per pair, and a
 * pair neither of whose lanes has data costs no state traffic.  A round never writes state it reads: when it finds more
 * runs than its device slab holds (silence against silence makes every diagonal a run) the slab grows to what was
 * counted and the round is repeated; nothing is lost and nothing is reported twice.
 * NEEDLE_HIP_CROSSMATCHER_RUN_SLAB=<runs> sets the initial slab (default 4096).
 *
 * Regions: openings and endings in one object (needle_hip_crossmatcher_new_regions).  The lanes are videos x regions,
 * regions = 1 or 2, lane = video * regions + region -- the numbering of the library's arena rows and of the comparator's
 * sequences with include_endings, and of needle_hip_feeder_frame_hashes(f, 2v, 2v + 1, ...).  Only lanes of one region
 * are matched against each other: the problem of pair (a, b) and region r is (src = lane a * R + r, dst = lane b * R + r,
 * min_len[r]) and NeedleHipRun.problem = pair * regions + r, so the complete list goes unchanged into
 * needle_hip_comparator_results_from_runs of a comparator with include_endings.  Every region has a capacity
 * max_items[r] and a min_len[r] of its own (the ending window is half the opening window); the entries of the state are
 * 2 bytes where every region's max_items is below 65 536, else 4, for the whole object.  Everything above holds per
 * (pair, region): the frontier of (a, b, r) is reported in the round in which the second of lanes a * R + r and
 * b * R + r finishes, whatever the other region does; a round is still three launches, one upload and one download.
 * needle_hip_crossmatcher_new is the regions = 1 case.  feed, finish, lane, ready, runs and stats work over the
 * videos * regions lanes: the arrays of feed have one entry per lane, feed_from_feeder wants a feeder of
 * videos * regions lanes, `complete` means every lane of every region is finished, stats[2] sums over regions and pairs.
 *
 * Resident videos: a new season joins a library (needle_hip_crossmatcher_new_resident).  K videos are known and complete,
 * N are arriving; the video list is the K resident videos followed by the N arriving ones, V = K + N (the index's append
 * order), so a resident is always the source of a pair with an arriving video.  The resident rows are given at creation as
 * the matcher takes its sources: one hash arena and one NeedleHipSeq per row k * regions + r; they are uploaded once, and
 * a row of 0 or 1 hashes is allowed and has no cells.  Only the arriving videos have lanes: lane = t * regions + r for
 * arriving video t, whose index among all videos is K + t; feed, finish, lane, feed_from_feeder (a feeder of N * regions
 * lanes), ready and shape work over these lanes as above.  The live problems are (a, b, r) with a < b and b >= K:
 *   resident x arriving (a < K): only the destination grows.  The state is the col frontier alone, one run length per
 *     resident row at the last column fed, sized by that row's own length and not by max_items, in two sets.  It costs
 *     (n_a - 1)(n_b - 1) cells, each evaluated once; no row-direction work is done for it.
 *   arriving x arriving (a >= K): the pair above, with its L frontier of 4 x max_items[r] entries.
 *   resident x resident: no state, no work, never reported.
 * NeedleHipRun.problem = pair_index(a, b, V) * regions + r with the indices among all V videos, in the comparator's
 * i-major order: pair_index = a (2 V - a - 1) / 2 + (b - a - 1).  Every pair of an arriving video is live, so the complete
 * list, given to needle_hip_comparator_results_from_runs(first_video = K, video_count = N) of a comparator over the V
 * videos, yields the arriving videos' results, those of a full search over all K + N videos.  The reporting rule is the
 * one above with Ja = n_a for a resident from the first round on: a run is reported in the round whose cells break it,
 * and what is open on a frontier -- a run into the resident's last row or into the lane's last column -- in the round in
 * which lane b finishes.  A round is still three launches, one upload and one download, whatever K is: the resident row
 * table (offset, length, state base) goes up once at creation, nothing per pair or per resident row in a round; a resident
 * problem whose arriving lane has no data and is not finishing leaves after its table reads, with no state traffic; a
 * round never writes state it reads, so the repeat after a slab overflow works as above.  The entries are 2 bytes where
 * every max_items[r] AND every resident row length is below 65 536, else 4, for the whole object.  min_len is per region,
 * a lower bound (the epilogue applies the duration test).  stats[2] counts the resident cells too.
 * Limits, checked before a device is asked for (InvalidArgument): regions 1 or 2; N 1..256 when K >= 1 (K = 0 is
 * needle_hip_crossmatcher_new_regions, N 2..256); max_items[r] in [2, 2^31 - 16]; every resident row inside the arena
 * (offset + len <= num_hashes) and len <= 2^31 - 16; min_len[r] >= 1; (K N + N (N - 1) / 2) x regions <= 65 535 live
 * problems (a grid dimension: 1 000 residents + 28 arriving x 2 regions = 56 756 fits, 2 000 + 28 x 2 regions does not:
 * beyond it a season goes through needle_hip_index_matcher_new / needle_hip_index_add_streamed below, at any library size);
 * V (V - 1) / 2 x regions < 2^32.  NULL arrays (hashes with num_hashes > 0, resident with num_resident > 0, max_items,
 * min_len) or a NULL output: NullArgument.
 *
 * Groups of videos: several shows decoded at once (needle_hip_crossmatcher_new_grouped).  The K resident and the N arriving
 * videos carry a 32-bit label each (any values: they are only compared; K may be 0 with the resident arguments NULL), the
 * video list is the residents first, and the live pairs are (a, b), a < b in list order, b >= K, with EQUAL labels.  Nothing
 * else is evaluated and no run of any other pair is ever reported, however alike two shows' jingles are.  Lanes, feeds,
 * finish, ready, lane, runs, stats, feed_from_feeder and the regions layout (lane = t * regions + r) are those above, and so
 * are exactness and the reporting rule, restricted to live pairs.  NeedleHipRun.problem = (grouped pair id over the V
 * labels) * regions + region: the numbering needle_hip_group_pairs decodes (groups in order of first appearance, inside a
 * group the i-major order over its members), so with K = 0 the complete list goes straight into
 * needle_hip_comparator_results_from_runs_grouped, and with one label and K = 0 the ids are those of
 * needle_hip_crossmatcher_new_regions.  A round is still three launches with nothing per pair uploaded: a live-pair table --
 * per live problem its two rows, its id and the place of its state -- is built on the host and uploaded once at creation,
 * next to the resident table.  State and hashes exist for live pairs only: an arriving pair's four frontier sets by its
 * number among the live arriving pairs; an (arriving t, resident k) col frontier only where the labels agree; a resident no
 * arriving video shares a label with has no hashes uploaded or gathered, no state, and is never read (it still counts in the
 * numbering, which is over all V).  Limits (InvalidArgument, before a device is asked for): regions 1 or 2; N 1..256; the
 * LIVE problems (same-label pairs with an arriving end, x regions) <= 65 535, whatever K is; the grouped pairs x regions
 * < 2^32; max_items, min_len and the resident rows as above.  A labelling without any live pair is allowed and reports
 * nothing.  NULL groups, or NULL resident / resident_groups with num_resident > 0: NullArgument.
 *
 * Out of scope: `reset`, `open`, more than two regions, several ranks.  Feeding the index, refreshed results for the
 * resident videos (their candidate lists also need the old pairs' entries, which the index holds) and resident rows taken
 * from a device arena are what needle_hip_index_crossmatcher_new / needle_hip_index_add_matched below do; a library too
 * large for the limit above takes the matcher route, needle_hip_index_matcher_new / needle_hip_index_add_streamed.
 *
 * lanes (videos) must be 2..256 (32 640 pairs: pair * regions + region is a grid dimension).  max_items >= 2 is the
 * capacity of every lane (of the region); state and histories are allocated at creation.  lanes, regions or max_items
 * out of range, min_len == 0, a feed that
 * would take a lane past max_items, items for a finished lane, a lane index out of range, unequal lane counts in
 * feed_from_feeder, first + count beyond the list in `runs`: InvalidArgument, checked for every lane before any device
 * work, so a refused feed moves no lane.  NULL handles and NULL outputs: NullArgument.  Without a HIP device creation
 * fails (there is no CPU path).  A device failure poisons the object: every later call returns it.  One thread at a
 * time per object. */
typedef struct NeedleHipCrossMatcher NeedleHipCrossMatcher;
enum NeedleError needle_hip_crossmatcher_new(size_t lanes, size_t max_items, uint32_t min_len, uint32_t threshold,
                                             NeedleHipCrossMatcher **output);
/* videos 2..256, regions 1..2; max_items[r] >= 2, min_len[r] >= 1 per region */
enum NeedleError needle_hip_crossmatcher_new_regions(size_t videos, size_t regions, const size_t *max_items, const uint32_t *min_len,
                                                     uint32_t threshold, NeedleHipCrossMatcher **output);
/* K = num_resident known videos (resident[k * regions + r] inside the arena `hashes`) in front of `videos` arriving ones;
 * num_resident == 0 is needle_hip_crossmatcher_new_regions */
enum NeedleError needle_hip_crossmatcher_new_resident(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *resident,
                                                      size_t num_resident, size_t videos, size_t regions, const size_t *max_items,
                                                      const uint32_t *min_len, uint32_t threshold, NeedleHipCrossMatcher **output);
/* groups of videos: resident_groups[k] and groups[t] are the labels of resident k and of arriving video t; only same-label
 * pairs with an arriving end are live; num_resident == 0: resident and resident_groups may be NULL */
enum NeedleError needle_hip_crossmatcher_new_grouped(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *resident,
                                                     size_t num_resident, const uint32_t *resident_groups, size_t videos,
                                                     const uint32_t *groups, size_t regions, const size_t *max_items,
                                                     const uint32_t *min_len, uint32_t threshold, NeedleHipCrossMatcher **output);
void needle_hip_crossmatcher_free(NeedleHipCrossMatcher *matcher);
/* one entry per lane, host hashes; num_items[i] == 0: nothing for lane i */
enum NeedleError needle_hip_crossmatcher_feed(NeedleHipCrossMatcher *matcher, const uint32_t *const *items, const size_t *num_items);
/* As the matcher's: lane by lane (equal lane counts) the feeder's ready items beyond items_fed; finishes the lanes the
 * feeder has finished. */
enum NeedleError needle_hip_crossmatcher_feed_from_feeder(NeedleHipCrossMatcher *matcher, NeedleHipFeeder *feeder);
enum NeedleError needle_hip_crossmatcher_finish(NeedleHipCrossMatcher *matcher, const size_t *lanes, size_t k); /* NULL: every unfinished lane */
/* num_runs: the length of the list; complete: every lane is finished (the list is final) */
enum NeedleError needle_hip_crossmatcher_ready(NeedleHipCrossMatcher *matcher, size_t *num_runs, bool *complete);
enum NeedleError needle_hip_crossmatcher_lane(NeedleHipCrossMatcher *matcher, size_t lane, uint64_t *items_fed, bool *finished);
enum NeedleError needle_hip_crossmatcher_runs(NeedleHipCrossMatcher *matcher, size_t first, size_t count, NeedleHipRun *runs);
/* stats[0] feeds that carried items, stats[1] kernel launches, stats[2] cells evaluated (host arithmetic of what the
 * kernel walks; a repeated round counts again), stats[3] bytes of device state: needle_hip_crossmatcher_state_bytes
 * plus the run slab. */
enum NeedleError needle_hip_crossmatcher_stats(const NeedleHipCrossMatcher *matcher, uint64_t stats[4]);
/* pure host arithmetic, no device: pairs x 2 sets x 2 x max_items x (2 or 4) + lanes x max_items x 4 bytes
 * (16.5 MB + 0.6 MB for 28 lanes of 5 441 items); 0 where lanes or max_items is out of range */
size_t needle_hip_crossmatcher_state_bytes(size_t lanes, size_t max_items);
/* the sum over the regions of pairs x 2 sets x 2 x max_items[r] x w + videos x max_items[r] x 4 bytes, w = 2 where every
 * max_items[r] < 65 536, else 4; 0 where an argument is out of range; regions = 1: needle_hip_crossmatcher_state_bytes */
size_t needle_hip_crossmatcher_state_bytes_regions(size_t videos, size_t regions, const size_t *max_items);
/* with P = N (N - 1) / 2 arriving pairs and S_r the sum of the resident lengths of region r, the sum over the regions of
 * P x 4 x max_items[r] x w + N x max_items[r] x 4 + N x 2 x S_r x w + S_r x 4 bytes; w = 2 where every max_items[r] and
 * every resident length < 65 536, else 4 (1 000 residents of 5 441, 28 arriving, one region: 648 218 976); the offsets of
 * `resident` are not looked at; 0 where an argument is out of range; num_resident = 0:
 * needle_hip_crossmatcher_state_bytes_regions.  stats[3] is this plus the resident table and the run slab. */
size_t needle_hip_crossmatcher_state_bytes_resident(const NeedleHipSeq *resident, size_t num_resident, size_t videos, size_t regions,
                                                    const size_t *max_items);
/* what needle_hip_crossmatcher_new_grouped allocates for frontiers and hashes, by host arithmetic: with P the live arriving
 * pairs, the sum over the regions of P x 4 x max_items[r] x w + N x max_items[r] x 4, plus per live (arriving t, resident k)
 * 2 x len(k, r) x w, plus 4 bytes per hash of a resident that is in a live pair; w = 2 where every max_items[r] and every
 * such resident's rows are below 65 536, else 4.  0 where the arguments are refused.  stats[3] of a grouped object is this
 * plus the live-pair table (24 bytes per live problem), the resident table and the run slab. */
size_t needle_hip_crossmatcher_state_bytes_grouped(const NeedleHipSeq *resident, size_t num_resident, const uint32_t *resident_groups,
                                                   size_t videos, const uint32_t *groups, size_t regions, const size_t *max_items);
/* the labels a grouped object was made with, residents first: n >= its residents + videos.  An ungrouped object:
 * NeedleError_InvalidArgument. */
enum NeedleError needle_hip_crossmatcher_groups(const NeedleHipCrossMatcher *matcher, uint32_t *labels, size_t n);
/* the resident videos the object was created with; 0 for needle_hip_crossmatcher_new and _new_regions */
enum NeedleError needle_hip_crossmatcher_resident(const NeedleHipCrossMatcher *matcher, size_t *num_resident);
/* what the object was created with (regions = 1 for needle_hip_crossmatcher_new): the arriving videos and the regions; it
 * has videos * regions lanes */
enum NeedleError needle_hip_crossmatcher_shape(const NeedleHipCrossMatcher *matcher, size_t *videos, size_t *regions);

/* ---- A streamed season into the index: its cross-matcher's runs in place of a second scan ------------------------
 * decoders -> feeder -> cross-matcher (made from the index) -> index.  needle_hip_index_crossmatcher_new makes the
 * object of needle_hip_crossmatcher_new_resident whose K resident videos are the index's, in the index's order: their rows
 * are gathered on the device from the index's hash arena (one launch; no hashes are uploaded, only the row table).
 * regions and threshold are the index's; max_items[r] and min_len[r] are the caller's.  The matcher remembers the index
 * (by an id from a process-wide counter) and the index's generation, which every successful add, remove, replace and
 * add_matched advances.
 *
 * needle_hip_index_add_matched appends the k = videos arriving videos of a complete matcher, with the runs it holds in
 * place of the scan.  Afterwards the index is what needle_hip_index_add(frame_hashes, k) leaves: the results of all
 * K + k videos (those of the K known ones refreshed), the same store, the same pairs_searched.  The run list goes up
 * once; one kernel re-tags it for the store and drops what the scan's problems exclude (a region one of whose rows can hold
 * no run long enough, a run shorter than max(min_len) of its two rows).  No pair is scanned: pairs_scanned *last = 0.
 * frame_hashes[t] is arriving video t (rows: lanes t * regions + r), e.g. from needle_hip_feeder_frame_hashes.
 *
 * Refused, before anything is committed and with the index exactly as it was (NeedleError_InvalidArgument unless noted):
 * a matcher not created from this index; a stale one (the index changed since its creation: a matcher is consumed once);
 * one that is not complete; k != its videos; a row whose length is not its lane's items_fed; a row whose hashes differ
 * from what the lane was fed (compared on the device); a min_len[r] above the smallest max(min_len) of a live pair whose
 * two rows can both hold a run (the matcher has then lost runs); a run that does not lie inside its rows; whatever
 * needle_hip_index_add refuses, in the same words; a poisoned matcher (its error); a matcher on another device.
 * NULL index, matcher, arrays or output: NeedleError_NullArgument. */
enum NeedleError needle_hip_index_crossmatcher_new(NeedleHipIndex *index, size_t videos, const size_t *max_items, const uint32_t *min_len,
                                                   NeedleHipCrossMatcher **output);
enum NeedleError needle_hip_index_add_matched(NeedleHipIndex *index, NeedleHipCrossMatcher *matcher,
                                              const FrameHashes *const *frame_hashes, size_t k);
/* ---- The same route into a grouped index: several shows' seasons streamed at once ---------------------------------
 * needle_hip_index_crossmatcher_new_grouped takes a grouped index, which may be empty, and makes the object of
 * needle_hip_crossmatcher_new_grouped: the residents are the index's videos in index order under the index's labels,
 * groups[t] is the label of arriving video t, and only the rows of the groups that arrive are gathered from the index's
 * arena.  The live problems are bounded by the arriving shows' sizes, not by the library's: (same-label pairs with an
 * arriving end) x regions <= 65 535.  needle_hip_index_add_matched_grouped appends the matcher's k arriving videos under the
 * matcher's labels with its runs in place of the scan; one kernel decodes each run's grouped id over all K + k videos and
 * re-tags it to the store's append-stable id, with the filter of needle_hip_index_add_matched.  Afterwards the index is
 * what needle_hip_index_add_grouped(frame_hashes, groups, k) leaves: results of all videos, evidence, store sizes,
 * pairs_searched, groups; pairs_scanned *last = 0.
 * Refused as needle_hip_index_add_matched refuses, in the same words, the index exactly as it was; and a plain index
 * (either call), a matcher without groups, a matcher whose resident labels are not the index's.
 * needle_hip_index_crossmatcher_new, _add_matched, _matcher_new and _add_streamed stay refused on a grouped index; the
 * matcher / add_streamed pair with groups is out of scope. */
enum NeedleError needle_hip_index_crossmatcher_new_grouped(NeedleHipIndex *index, size_t videos, const uint32_t *groups, const size_t *max_items,
                                                           const uint32_t *min_len, NeedleHipCrossMatcher **output);
enum NeedleError needle_hip_index_add_matched_grouped(NeedleHipIndex *index, NeedleHipCrossMatcher *matcher,
                                                      const FrameHashes *const *frame_hashes, size_t k);
/* ---- A streamed season into an index of any size: a matcher made from the index, and the arriving pairs' cross-matcher --
 * The cross-matcher above holds (K N + N (N - 1) / 2) x regions live problems in a grid dimension, so a large index cannot
 * make one.  The second route splits the new pairs:
 *   resident x arriving: needle_hip_index_matcher_new makes the object of needle_hip_matcher_new_regions whose sources are
 *     the index's K x regions rows, in the index's order (source = video * regions + region), gathered on the device from
 *     the index's hash arena (one launch; only tables are uploaded).  regions and threshold are the index's; a source's
 *     min_len is the row's own shortest run that can pass the duration test, a lower bound for every pair the row is in (0:
 *     the row can hold none and has no cells).  It has videos x regions lanes, lane = t * regions + r for arriving video t,
 *     and remembers the index and its generation.  K is not bounded; videos x regions <= 65 535.  An empty index has nothing
 *     resident: InvalidArgument (a first season goes through needle_hip_index_crossmatcher_new).
 *   arriving x arriving: a cross-matcher without residents over the same k videos, needle_hip_crossmatcher_new_regions with
 *     the index's regions and threshold (k <= 256); NULL only when k == 1.
 * One feeder of videos x regions lanes feeds both (feed_from_feeder): each takes from its own items_fed on.
 *
 * needle_hip_index_add_streamed appends the k arriving videos with both run lists in place of the scan.  One kernel re-tags
 * them for the store -- a matcher run with problem = resident * regions + r on lane t * regions + r is pair (resident,
 * K + t), a cross-matcher run of i-major pair (a, b) over the k videos is pair (K + a, K + b) -- and drops what the scan's
 * problems exclude.  Afterwards the index is what needle_hip_index_add(frame_hashes, k) leaves: the results of all K + k
 * videos, the same store, the same pairs_searched; pairs_scanned *last = 0.  When to take which: one cross-matcher
 * (needle_hip_index_add_matched) while its live problems fit, this route beyond.
 *
 * Refused, before anything is committed and with the index exactly as it was (NeedleError_InvalidArgument unless noted),
 * for either object where it applies: a matcher not created from this index; a stale one; another device; an object that is
 * not complete (every lane finished); lane counts other than k x regions; a row whose length is not its lane's items_fed;
 * a row whose hashes differ from either object's history for that lane (compared on the device); a run that does not lie
 * inside its rows; a cross-matcher min_len[r] above the smallest max(min_len) of an arriving pair whose two rows can both
 * hold a run; a cross-matcher that has residents; a NULL cross-matcher with k > 1; whatever needle_hip_index_add refuses,
 * in the same words; a poisoned object (its error).  NULL index, matcher, array or output: NeedleError_NullArgument. */
enum NeedleError needle_hip_index_matcher_new(NeedleHipIndex *index, size_t videos, NeedleHipMatcher **output);
enum NeedleError needle_hip_index_add_streamed(NeedleHipIndex *index, NeedleHipMatcher *matcher, NeedleHipCrossMatcher *crossmatcher,
                                               const FrameHashes *const *frame_hashes, size_t k);
/* Video pairs handed to the one-shot scan: over the index's life (*total) and by the last successful operation (*last: 0
 * after add_matched, add_streamed and remove).  needle_hip_index_pairs_searched counts the pairs that entered the index either way.
 * Either pointer may be NULL. */
enum NeedleError needle_hip_index_pairs_scanned(const NeedleHipIndex *index, uint64_t *total, uint64_t *last);

/* ---- Compressed fingerprints: chromaprint 1.5's FingerprintCompressor / FingerprintDecompressor on the device ----
 * The string `fpcalc` prints and databases store.  x[i] = item[i] ^ item[i-1] (item[-1] = 0); the set bits of x from bit 0
 * up, at 1-based positions p, as gaps to the previous one: gap < 7 is the 3-bit symbol gap, gap >= 7 the symbol 7 and a
 * 5-bit exceptional symbol gap - 7; the symbol 0 ends the item.  A blob is [algorithm & 0xFF] [n >> 16] [n >> 8] [n], the
 * 3-bit symbols packed LSB first into ceil(3 S / 8) bytes, then the 5-bit ones into ceil(5 E / 8) bytes, padding bits 0.
 * The text form is base64 with the URL-safe alphabet and no padding.
 *
 * The codec is batched: fingerprint b is items[item_offsets[b] .. item_offsets[b + 1]), blob b is
 * blobs[blob_offsets[b] .. blob_offsets[b + 1]); offsets rows have count + 1 entries and must not decrease
 * (InvalidArgument).  Output buffers are malloc'd (needle_hip_host_free); the offsets rows, `algorithms` and `status`
 * are the caller's.  There is no CPU codec: without a device the compute calls fail as every other one does.
 *
 * compress: a fingerprint of 2^24 items or more is InvalidArgument with nothing done (the header has 24 bits).
 * decompress: status[b] is 0 ok; 1 the blob is shorter than a header; 2 the 3-bit stream ends before n terminators, or
 * the header claims more items than the blob's bytes can hold (floor(8 (L - 4) / 3): refused before anything is
 * allocated); 3 the exceptional stream ends early; 4 a bit position above 32.  A refused blob has an empty slot
 * (item_offsets[b + 1] == item_offsets[b]) and the call returns Ok.  Bytes behind the exceptional stream are ignored, as
 * upstream ignores them.  algorithms[b] is the blob's first byte (0 for an empty blob).  A blob longer than 2^30 bytes
 * is InvalidArgument.
 * feeder_compressed: the blob of a finished lane's kept items; an unfinished lane is InvalidArgument.
 * compressed_bound, base64_encode / _decode, codec_tiles and simhash are pure host.  base64_decode refuses (InvalidArgument)
 * characters outside the alphabet and a length of 1 mod 4; encode's text is NUL-terminated, *size excludes the NUL.
 * codec_tiles: the items of a compress tile and the 3-bit symbols of a decompress tile, for tests that sit on their edges.
 * simhash: chromaprint's 32-bit simhash of a fingerprint (what the run reports carry), 0 for an empty one. */
size_t needle_hip_fingerprint_compressed_bound(size_t items); /* 4 + ceil(99 n / 8) + ceil(20 n / 8) */
enum NeedleError needle_hip_fingerprint_compress_host(const uint32_t *items, const uint64_t *item_offsets, size_t count, int algorithm,
                                                      uint8_t **blobs, uint64_t *blob_offsets);
enum NeedleError needle_hip_fingerprint_decompress_host(const uint8_t *blobs, const uint64_t *blob_offsets, size_t count, uint32_t **items,
                                                        uint64_t *item_offsets, int32_t *algorithms, int32_t *status);
enum NeedleError needle_hip_feeder_compressed(NeedleHipFeeder *feeder, size_t lane, int algorithm, uint8_t **blob, size_t *size);
enum NeedleError needle_hip_fingerprint_base64_encode(const uint8_t *data, size_t size, char **text, size_t *text_size);
enum NeedleError needle_hip_fingerprint_base64_decode(const char *text, size_t text_size, uint8_t **data, size_t *size);
enum NeedleError needle_hip_fingerprint_codec_tiles(size_t *compress_items, size_t *decompress_symbols);
enum NeedleError needle_hip_fingerprint_simhash(const uint32_t *items, size_t count, uint32_t *hash);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLE_HIP_H */
