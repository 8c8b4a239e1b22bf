// extern "C" surface of libneedle_capi.so.
//   * the 13 needle-capi symbols (include/needle.h; reference: needle-capi/src/lib.rs)
//   * the additive needle_hip_* entry points (include/needle_hip.h)
// Nothing throws across this boundary: every body is wrapped, and failures become NeedleError codes
// with the detail printed as "needle error: ..." on stderr (lib.rs:124).
#include <dirent.h>
#include <hip/hip_runtime_api.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <fstream>
#include <new>

#include "crossmatch.h"
#include "epilogue.h"
#include "hipctx.h"
#include "feeder.h"
#include "fp_codec.h"
#include "index.h"
#include "matcher.h"
#include "needle_core.h"

using namespace needle;

// ---- opaque handle types (lib.rs:308,347-350,531) ----------------------------------------------------------
struct FrameHashes {
  FrameHashesData d;
};
struct NeedleAudioAnalyzer {
  Analyzer inner;
  std::vector<FrameHashes> frame_hashes;
};
struct NeedleAudioComparator {
  Comparator inner;
};
struct NeedleHipFeeder {
  std::unique_ptr<Feeder> inner;
};
struct NeedleHipMatcher {
  std::unique_ptr<Matcher> inner;
};
struct NeedleHipCrossMatcher {
  std::unique_ptr<CrossMatcher> inner;
};
struct NeedleHipIndex {
  explicit NeedleHipIndex(const Comparator &c, bool grouped = false) : inner(c, grouped) {}
  Index inner;
};

namespace {

template <typename F>
NeedleError guarded(F &&f) {
  try {
    return f();
  } catch (const std::bad_alloc &) {
    return report(Status::Make(NeedleError_Unknown, "out of memory"));
  } catch (const std::exception &e) {
    return report(Status::Make(NeedleError_Unknown, std::string("internal error: ") + e.what()));
  } catch (...) {
    return report(Status::Make(NeedleError_Unknown, "internal error"));
  }
}

bool valid_utf8(const char *s) {
  const unsigned char *p = reinterpret_cast<const unsigned char *>(s);
  while (*p) {
    int extra;
    unsigned cp;
    if (*p < 0x80) {
      p++;
      continue;
    } else if ((*p & 0xE0) == 0xC0) {
      extra = 1;
      cp = *p & 0x1F;
    } else if ((*p & 0xF0) == 0xE0) {
      extra = 2;
      cp = *p & 0x0F;
    } else if ((*p & 0xF8) == 0xF0) {
      extra = 3;
      cp = *p & 0x07;
    } else {
      return false;
    }
    p++;
    for (int i = 0; i < extra; i++, p++) {
      if ((*p & 0xC0) != 0x80) return false;
      cp = (cp << 6) | (*p & 0x3F);
    }
    if ((extra == 1 && cp < 0x80) || (extra == 2 && cp < 0x800) || (extra == 3 && cp < 0x10000) || cp > 0x10FFFF ||
        (cp >= 0xD800 && cp <= 0xDFFF))
      return false;
  }
  return true;
}

// get_paths_from_raw, lib.rs:283-304
NeedleError paths_from_raw(const char *const *raw, size_t n, std::vector<std::string> *out) {
  for (size_t i = 0; i < n; i++) {
    if (!raw[i]) return NeedleError_NullArgument;
    if (!valid_utf8(raw[i])) return NeedleError_InvalidUtf8String;
    out->emplace_back(raw[i]);
  }
  return NeedleError_Ok;
}

bool ends_with(const std::string &s, const std::string &suffix) {
  return s.size() >= suffix.size() && s.compare(s.size() - suffix.size(), suffix.size(), suffix) == 0;
}

// util.rs:22-53 with this build's notion of a decodable file: RIFF/WAVE.  (Upstream sniffs video
// containers with `infer` / FFmpeg; media decode is outside the analyze/search path built here.)
bool is_valid_media_file(const std::string &path, bool full) {
  if (ends_with(path, FRAME_HASH_DATA_FILE_NAME)) return false;
  struct stat st;
  if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return false;
  std::ifstream f(path, std::ios::binary);
  char head[12] = {0};
  f.read(head, 12);
  if (f.gcount() != 12 || std::memcmp(head, "RIFF", 4) != 0 || std::memcmp(head + 8, "WAVE", 4) != 0) return false;
  if (!full) return true;
  WavInfo w;  // `full`: the header has to describe an encoding this build decodes (util.rs:33-49 opens the demuxer)
  return wav_probe(path, &w).ok();
}

void fill_result(const VideoResult &v, NeedleHipSearchResult *r) {
  std::memset(r, 0, sizeof(*r));
  r->has_result = v.has_result;
  r->has_opening = v.result.has_opening;
  r->has_ending = v.result.has_ending;
  r->opening_start_ns = v.result.opening_start;
  r->opening_end_ns = v.result.opening_end;
  r->ending_start_ns = v.result.ending_start;
  r->ending_end_ns = v.result.ending_end;
}

}  // namespace

extern "C" {

// ============================================================================================================
// needle.h
// ============================================================================================================
const char *needle_error_to_str(enum NeedleError error) {  // lib.rs:138-199
  switch (error) {
    case NeedleError_Ok: return "No error";
    case NeedleError_InvalidUtf8String: return "Invalid UTF-8 string";
    case NeedleError_NullArgument: return "Input argument is NULL";
    case NeedleError_InvalidArgument: return "One or more input arguments were invalid (usually zero)";
    case NeedleError_FrameHashDataNotFound: return "Frame hash data not found on disk";
    case NeedleError_FrameHashDataInvalidVersion: return "Frame hash data has an invalid version.";
    case NeedleError_InvalidFrameHashData: return "Invalid frame hash data read from disk";
    case NeedleError_ComparatorMinimumPaths: return "Comparator requires at least 2 video paths";
    case NeedleError_AnalyzerInvalidHashPeriod: return "Analyzer hash period must be greater than 0";
    case NeedleError_AnalyzerInvalidHashDuration: return "Analyzer hash duration must be greater than 3 seconds";
    case NeedleError_IOError: return "I/O error";
    case NeedleError_Unknown: break;
  }
  return "Unknown error occurred; please re-run with logging enabled";
}

enum NeedleError needle_util_find_video_files(const char *const *paths, size_t num_paths, bool full, bool audio,
                                              const char *const **videos, size_t *num_videos) {
  (void)audio;  // every decodable file here is audio
  if (!paths || !videos || !num_videos) return NeedleError_NullArgument;  // lib.rs:216-218
  if (num_paths == 0) return NeedleError_InvalidArgument;                // lib.rs:219-221
  return guarded([&]() -> NeedleError {
    std::vector<std::string> in;
    NeedleError e = paths_from_raw(paths, num_paths, &in);
    if (e != NeedleError_Ok) return e;
    struct stat st;
    for (const std::string &p : in)  // util.rs:66-71 -> Error::PathNotFound -> Unknown (lib.rs:131)
      if (stat(p.c_str(), &st) != 0)
        return report(Status::Make(NeedleError_Unknown, "path does not exist: \"" + p + "\""));
    std::vector<std::string> found;
    for (const std::string &p : in) {
      stat(p.c_str(), &st);
      if (S_ISDIR(st.st_mode)) {  // one level deep, util.rs:77-88
        std::vector<std::string> names;
        if (DIR *d = opendir(p.c_str())) {
          while (dirent *ent = readdir(d)) {
            const std::string name = ent->d_name;
            if (name != "." && name != "..") names.push_back(name);
          }
          closedir(d);
        }
        std::sort(names.begin(), names.end());
        for (const std::string &name : names) {
          const std::string child = (ends_with(p, "/") ? p : p + "/") + name;
          if (is_valid_media_file(child, full)) found.push_back(child);
        }
      } else if (is_valid_media_file(p, full)) {
        found.push_back(p);
      }
    }
    char **arr = static_cast<char **>(std::malloc(std::max<size_t>(found.size(), 1) * sizeof(char *)));
    if (!arr) return report(Status::Make(NeedleError_Unknown, "out of memory"));
    for (size_t i = 0; i < found.size(); i++) arr[i] = strdup(found[i].c_str());
    *videos = const_cast<const char *const *>(arr);
    *num_videos = found.size();
    return NeedleError_Ok;
  });
}

void needle_util_video_files_free(const char *const *videos, size_t num_videos) {  // lib.rs:259-281
  if (!videos || num_videos == 0) return;
  char **arr = const_cast<char **>(videos);
  for (size_t i = 0; i < num_videos; i++) std::free(arr[i]);
  std::free(arr);
}

enum NeedleError needle_audio_analyzer_new(const char *const *paths, size_t num_paths,
                                           float opening_search_percentage, float ending_search_percentage,
                                           bool include_endings, bool threaded_decoding, bool force,
                                           struct NeedleAudioAnalyzer **output) {
  if (!paths || !output) return NeedleError_NullArgument;  // lib.rs:383-385
  return guarded([&]() -> NeedleError {
    std::vector<std::string> p;
    NeedleError e = paths_from_raw(paths, num_paths, &p);
    if (e != NeedleError_Ok) return e;
    auto *a = new NeedleAudioAnalyzer();
    a->inner = Analyzer::from_files(std::move(p), threaded_decoding, force);
    a->inner.with_opening_search_percentage(opening_search_percentage)
        .with_ending_search_percentage(ending_search_percentage)
        .with_include_endings(include_endings);
    *output = a;
    return NeedleError_Ok;
  });
}

enum NeedleError needle_audio_analyzer_new_default(const char *const *paths, size_t num_paths,
                                                   struct NeedleAudioAnalyzer **output) {  // lib.rs:354-369
  return needle_audio_analyzer_new(paths, num_paths, DEFAULT_OPENING_SEARCH_PERCENTAGE,
                                   DEFAULT_ENDING_SEARCH_PERCENTAGE, false, false, false, output);
}

enum NeedleError needle_audio_analyzer_get_frame_hashes(const struct NeedleAudioAnalyzer *analyzer, size_t index,
                                                        const struct FrameHashes **output) {  // lib.rs:415-435
  if (!analyzer || !output) return NeedleError_NullArgument;
  if (index >= analyzer->frame_hashes.size()) return NeedleError_InvalidArgument;
  *output = &analyzer->frame_hashes[index];
  return NeedleError_Ok;
}

void needle_audio_analyzer_free(const struct NeedleAudioAnalyzer *analyzer) {  // lib.rs:439-446
  delete const_cast<NeedleAudioAnalyzer *>(analyzer);
}

void needle_audio_analyzer_print_paths(const struct NeedleAudioAnalyzer *analyzer) {  // lib.rs:450-461
  if (!analyzer) return;
  for (const std::string &p : analyzer->inner.videos()) std::printf("%s\n", p.c_str());
  std::fflush(stdout);
}

enum NeedleError needle_audio_analyzer_run(struct NeedleAudioAnalyzer *analyzer, float hash_duration, bool persist,
                                           bool threading) {  // lib.rs:465-491
  if (!analyzer) return NeedleError_NullArgument;
  if (!(hash_duration > 0.0f)) return NeedleError_AnalyzerInvalidHashDuration;  // lib.rs:474-476
  return guarded([&]() -> NeedleError {
    bool ok = true;
    const ns_t hd = duration_from_secs_f32(hash_duration, &ok);
    if (!ok) return NeedleError_AnalyzerInvalidHashDuration;
    std::vector<FrameHashesData> out;
    Status s = analyzer->inner.run(hd, persist, threading, &out);
    if (!s.ok()) return report(s);
    analyzer->frame_hashes.clear();
    for (FrameHashesData &d : out) analyzer->frame_hashes.push_back(FrameHashes{std::move(d)});
    return NeedleError_Ok;
  });
}

enum NeedleError needle_audio_comparator_new(const char *const *paths, size_t num_paths, bool include_endings,
                                             uint16_t hash_match_threshold, uint16_t min_opening_duration,
                                             uint16_t min_ending_duration, float time_padding,
                                             const struct NeedleAudioComparator **output) {  // lib.rs:556-597
  if (!paths || !output) return NeedleError_NullArgument;
  if (num_paths < 2) return NeedleError_ComparatorMinimumPaths;
  return guarded([&]() -> NeedleError {
    std::vector<std::string> p;
    NeedleError e = paths_from_raw(paths, num_paths, &p);
    if (e != NeedleError_Ok) return e;
    bool ok = true;
    const ns_t pad = duration_from_secs_f32(time_padding, &ok);  // Duration::from_secs_f32 panics on bad input
    if (!ok) return report(Status::Make(NeedleError_InvalidArgument, "time_padding must be a finite, non-negative number"));
    auto *c = new NeedleAudioComparator();
    c->inner = Comparator::from_files(std::move(p));
    c->inner.with_include_endings(include_endings)
        .with_hash_match_threshold(hash_match_threshold)
        .with_min_opening_duration((ns_t)min_opening_duration * kNanosPerSec)
        .with_min_ending_duration((ns_t)min_ending_duration * kNanosPerSec)
        .with_time_padding(pad);
    *output = c;
    return NeedleError_Ok;
  });
}

enum NeedleError needle_audio_comparator_new_default(const char *const *paths, size_t num_paths,
                                                     const struct NeedleAudioComparator **output) {  // lib.rs:537-552
  return needle_audio_comparator_new(paths, num_paths, false, DEFAULT_HASH_MATCH_THRESHOLD,
                                     DEFAULT_MIN_OPENING_DURATION, DEFAULT_MIN_ENDING_DURATION, 0.0f, output);
}

void needle_audio_comparator_free(const struct NeedleAudioComparator *comparator) {  // lib.rs:601-608
  delete const_cast<NeedleAudioComparator *>(comparator);
}

enum NeedleError needle_audio_comparator_run(const struct NeedleAudioComparator *comparator, bool analyze,
                                             bool display, bool use_skip_files, bool write_skip_files,
                                             bool threading) {  // lib.rs:612-637
  if (!comparator) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    const bool trace = std::getenv("NEEDLE_HIP_TRACE") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<VideoResult> res;
    Status s = comparator->inner.run(analyze, display, use_skip_files, write_skip_files, threading, &res);
    if (trace)
      std::fprintf(stderr, "[needle_hip] comparator run, whole call: %.2f ms\n",
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

// ============================================================================================================
// needle_hip.h — device / diagnostics
// ============================================================================================================
enum NeedleError needle_hip_device_count(int *count) {
  if (!count) return NeedleError_NullArgument;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  *count = n;
  return NeedleError_Ok;
}

enum NeedleError needle_hip_set_device(int ordinal) {
  return guarded([&]() -> NeedleError {
    Status s = ensure_device();
    if (!s.ok()) return report(s);
    if (hipSetDevice(ordinal) != hipSuccess) {
      (void)hipGetLastError();
      return report(Status::Make(NeedleError_InvalidArgument, "no such HIP device: " + std::to_string(ordinal)));
    }
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_device_pci_bus_id(char out[32]) {
  if (!out) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = ensure_device();
    if (!s.ok()) return report(s);
    int dev = 0;
    out[0] = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetPCIBusId(out, 32, dev) != hipSuccess) {
      (void)hipGetLastError();
      return report(Status::Make(NeedleError_Unknown, "the HIP runtime did not name the device's PCI address"));
    }
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_synchronize(void) {
  return guarded([&]() -> NeedleError {
    Status s = ensure_device();
    if (!s.ok()) return report(s);
    if (hipStreamSynchronize(library_stream()) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      return report(Status::Make(NeedleError_Unknown, std::string("HIP error: ") + hipGetErrorString(hipGetLastError())));
    return NeedleError_Ok;
  });
}

void *needle_hip_stream(void) {
  void *out = nullptr;
  guarded([&]() -> NeedleError {
    Status s = ensure_device();
    if (!s.ok()) return report(s);
    out = reinterpret_cast<void *>(library_stream());
    return NeedleError_Ok;
  });
  return out;
}

const char *needle_hip_last_error_message(void) { return last_error(); }
const char *needle_hip_version(void) { return "needle-mi355x 0.1.0 (gfx950, f64 fingerprint, exact integer search)"; }

enum NeedleError needle_hip_malloc(void **device_ptr, size_t bytes) {
  if (!device_ptr) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = ensure_device();
    if (!s.ok()) return report(s);
    if (hipMalloc(device_ptr, bytes ? bytes : 1) != hipSuccess)
      return report(Status::Make(NeedleError_Unknown, "hipMalloc failed for " + std::to_string(bytes) + " bytes"));
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_free(void *device_ptr) {
  if (device_ptr && hipFree(device_ptr) != hipSuccess) return report(Status::Make(NeedleError_Unknown, "hipFree failed"));
  return NeedleError_Ok;
}

enum NeedleError needle_hip_memcpy_h2d(void *device_dst, const void *host_src, size_t bytes) {
  if (!device_dst || !host_src) return NeedleError_NullArgument;
  hipStream_t st = library_stream();
  if (hipMemcpyAsync(device_dst, host_src, bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return report(Status::Make(NeedleError_Unknown, "host-to-device copy failed"));
  return NeedleError_Ok;
}

enum NeedleError needle_hip_memcpy_d2h(void *host_dst, const void *device_src, size_t bytes) {
  if (!host_dst || !device_src) return NeedleError_NullArgument;
  hipStream_t st = library_stream();
  if (hipMemcpyAsync(host_dst, device_src, bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return report(Status::Make(NeedleError_Unknown, "device-to-host copy failed"));
  return NeedleError_Ok;
}

void needle_hip_host_free(void *ptr) { std::free(ptr); }

enum NeedleError needle_hip_host_alloc(void **host_ptr, size_t bytes) {
  if (!host_ptr) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = ensure_device();
    if (!s.ok()) return report(s);
    if (hipHostMalloc(host_ptr, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess)
      return report(Status::Make(NeedleError_Unknown, "pinned allocation of " + std::to_string(bytes) + " bytes failed"));
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_host_alloc_free(void *host_ptr) {
  if (host_ptr && hipHostFree(host_ptr) != hipSuccess) return report(Status::Make(NeedleError_Unknown, "hipHostFree failed"));
  return NeedleError_Ok;
}

enum NeedleError needle_hip_fingerprint_cert_stats(uint64_t counts[4], bool reset) {
  if (!counts) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = gpu_fingerprint_cert_stats(counts, reset);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_scan_issued_evaluations(uint64_t *lane_evaluations, bool reset) {
  if (!lane_evaluations) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = gpu_scan_issued_evaluations(lane_evaluations, reset);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_scan_counts(uint64_t counts[2], bool reset) {
  if (!counts) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = gpu_scan_issued_evaluations(&counts[0], reset, &counts[1]);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_scan_last_launch(int32_t *form, uint64_t *matrix_products) {
  if (!form || !matrix_products) return NeedleError_NullArgument;
  gpu_scan_last_launch(form, matrix_products);
  return NeedleError_Ok;
}

enum NeedleError needle_hip_epilogue_host_fallbacks(uint64_t *jobs, bool reset) {
  if (!jobs) return NeedleError_NullArgument;
  *jobs = reset ? epilogue_host_fallbacks().exchange(0) : epilogue_host_fallbacks().load();
  return NeedleError_Ok;
}

enum NeedleError needle_hip_int_valu_ceiling(double *cells_per_second) {
  if (!cells_per_second) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = gpu_int_valu_ceiling(cells_per_second);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

double needle_hip_last_kernel_ms(const char *kernel) { return kernel ? kernel_ms(kernel) : -1.0; }
void needle_hip_set_kernel_timing(const char *kernels) { set_kernel_timing(kernels); }
size_t needle_hip_kernel_launches(const char *kernel) { return kernel ? kernel_launches(kernel) : 0; }

// ============================================================================================================
// fingerprint
// ============================================================================================================
int needle_hip_fingerprint_sample_rate(void) { return kSampleRate; }
int needle_hip_fingerprint_delay_ms(void) { return kDelayMs; }
int needle_hip_fingerprint_item_duration_ms(void) { return kItemDurationMs; }
size_t needle_hip_fingerprint_num_items(size_t samples_per_channel) { return num_items(samples_per_channel); }
size_t needle_hip_fingerprint_num_kept(size_t samples_per_channel, uint32_t step) {
  return num_kept(samples_per_channel, step);
}

enum NeedleError needle_hip_fingerprint_host(const int16_t *const *pcm, const size_t *num_values, size_t num_streams,
                                             int channels, uint32_t step, uint32_t *const *items) {
  if (!pcm || !num_values || !items) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const int16_t *> p(pcm, pcm + num_streams);
    std::vector<size_t> n(num_values, num_values + num_streams);
    for (size_t i = 0; i < num_streams; i++)
      if ((!p[i] && n[i]) || !items[i]) return NeedleError_NullArgument;
    std::vector<std::vector<uint32_t>> out;
    Status s = gpu_fingerprint_host(p, n, channels, step, &out);
    if (!s.ok()) return report(s);
    for (size_t i = 0; i < num_streams; i++)
      if (!out[i].empty()) std::memcpy(items[i], out[i].data(), out[i].size() * sizeof(uint32_t));
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_fingerprint_device(const int16_t *d_pcm, const uint64_t *pcm_offsets,
                                               const uint64_t *num_values, size_t num_streams, int channels,
                                               uint32_t step, uint32_t *d_items, const uint64_t *item_offsets,
                                               bool sync) {
  if (!d_pcm || !pcm_offsets || !num_values || !d_items || !item_offsets) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<StreamSpan> spans(num_streams);
    for (size_t i = 0; i < num_streams; i++) spans[i] = StreamSpan{pcm_offsets[i], num_values[i], item_offsets[i]};
    Status s = gpu_fingerprint_device(d_pcm, spans, channels, step, d_items, sync);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_fingerprint_audit_device(const int16_t *d_pcm, const uint64_t *pcm_offsets, const uint64_t *num_values,
                                                     size_t num_streams, int channels, uint32_t step, const uint32_t *d_items,
                                                     const uint64_t *item_offsets, NeedleHipCertAudit *audit) {
  if (!d_pcm || !pcm_offsets || !num_values || !d_items || !item_offsets || !audit) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<StreamSpan> spans(num_streams);
    for (size_t i = 0; i < num_streams; i++) spans[i] = StreamSpan{pcm_offsets[i], num_values[i], item_offsets[i]};
    uint64_t c[4] = {0, 0, 0, 0};
    Status s = gpu_fingerprint_audit_device(d_pcm, spans, channels, step, d_items, c, &audit->max_error_over_s, &audit->max_s);
    if (!s.ok()) return report(s);
    audit->items = c[0];
    audit->accepted = c[1];
    audit->accepted_mismatches = c[2];
    audit->mismatches = c[3];
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_fingerprint_debug(const int16_t *pcm, size_t num_values, int channels, double *chroma,
                                              double *features) {
  if (!pcm) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = ensure_device();
    if (!s.ok()) return report(s);
    if (channels != 1 && channels != 2) return NeedleError_InvalidArgument;
    const size_t samples = num_values / (size_t)channels;
    const size_t frames = num_frames(samples), rows = frames >= 5 ? frames - 4 : 0, kept = num_items(samples);
    DeviceBuffer<int16_t> d_pcm;
    DeviceBuffer<uint32_t> d_items;
    DeviceBuffer<double> d_chroma, d_feat;
    if (!(s = d_pcm.reserve(std::max<size_t>(num_values, 1))).ok()) return report(s);
    if (!(s = d_items.reserve(std::max<size_t>(kept, 1))).ok()) return report(s);
    if (!(s = d_chroma.reserve(std::max<size_t>(frames, 1) * kBands)).ok()) return report(s);
    if (!(s = d_feat.reserve(std::max<size_t>(rows, 1) * kBands)).ok()) return report(s);
    if (hipMemcpy(d_pcm.ptr, pcm, num_values * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess)
      return report(Status::Make(NeedleError_Unknown, "host-to-device copy failed"));
    std::vector<StreamSpan> spans{StreamSpan{0, num_values, 0}};
    s = gpu_fingerprint_device(d_pcm.ptr, spans, channels, 1, d_items.ptr, true, d_chroma.ptr, d_feat.ptr);
    if (!s.ok()) return report(s);
    if (chroma && frames && hipMemcpy(chroma, d_chroma.ptr, frames * kBands * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return report(Status::Make(NeedleError_Unknown, "device-to-host copy failed"));
    if (features && rows && hipMemcpy(features, d_feat.ptr, rows * kBands * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return report(Status::Make(NeedleError_Unknown, "device-to-host copy failed"));
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_fingerprint_stages_debug(const int16_t *const *pcm, const size_t *num_values, size_t num_streams,
                                                     int channels, uint32_t step, uint32_t flags, NeedleHipStages *stages) {
  if (!stages || (num_streams && (!pcm || !num_values))) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const int16_t *> p(pcm, pcm + num_streams);
    std::vector<size_t> n(num_values, num_values + num_streams);
    for (size_t i = 0; i < num_streams; i++)
      if (!p[i] && n[i]) return NeedleError_NullArgument;
    Status s = gpu_fingerprint_stages_debug(p, n, channels, step, flags, stages);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

// ============================================================================================================
// resampler front-end
// ============================================================================================================
size_t needle_hip_resample_out_len(size_t samples_per_channel, int sample_rate) {
  return sample_rate > 0 ? resample_out_len(samples_per_channel, sample_rate) : 0;
}

enum NeedleError needle_hip_resample_plan(int sample_rate, NeedleHipResamplePlan *out) {
  if (!out) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = resample_plan_host(sample_rate, out);
    if (!s.ok()) set_last_error(s.message);  // (not printed: a refusal is this query's answer, and a sweep asks 766 001 times)
    return s.code;
  });
}

enum NeedleError needle_hip_resample_host(const int16_t *const *pcm, const size_t *num_values, size_t num_streams,
                                          int channels, int sample_rate, int16_t *const *out) {
  if (!pcm || !num_values || !out) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const int16_t *> p(pcm, pcm + num_streams);
    std::vector<size_t> n(num_values, num_values + num_streams);
    for (size_t i = 0; i < num_streams; i++)
      if ((!p[i] && n[i]) || !out[i]) return NeedleError_NullArgument;
    std::vector<std::vector<int16_t>> res;
    Status s = gpu_resample_host(p, n, channels, sample_rate, &res);
    if (!s.ok()) return report(s);
    for (size_t i = 0; i < num_streams; i++)
      if (!res[i].empty()) std::memcpy(out[i], res[i].data(), res[i].size() * sizeof(int16_t));
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_downmix_host(const int16_t *const *pcm, const size_t *num_values, size_t num_streams,
                                         int channels, int16_t *const *out) {
  if (!pcm || !num_values || !out) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const int16_t *> p(pcm, pcm + num_streams);
    std::vector<size_t> n(num_values, num_values + num_streams);
    std::vector<int16_t *> o(out, out + num_streams);
    for (size_t i = 0; i < num_streams; i++)
      if ((!p[i] && n[i]) || (!o[i] && channels > 0 && n[i] >= (size_t)channels)) return NeedleError_NullArgument;
    Status s = gpu_downmix_host(p, n, channels, o);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_convert_host(const void *const *pcm, const size_t *num_values, size_t num_streams, int channels,
                                         int format, int16_t *const *out) {
  if (!pcm || !num_values || !out) return NeedleError_NullArgument;
  if (channels < 1 || channels > NEEDLE_HIP_MAX_CHANNELS || !sample_format_valid(format)) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    const size_t planes = sample_format_planes(format, channels);
    std::vector<const void *> p(pcm, pcm + num_streams * planes);
    std::vector<size_t> n(num_values, num_values + num_streams);
    std::vector<int16_t *> o(out, out + num_streams);
    for (size_t i = 0; i < num_streams; i++) {
      if (n[i] < (size_t)channels) continue;  // no whole frame: nothing is read or written
      if (!o[i]) return NeedleError_NullArgument;
      for (size_t c = 0; c < planes; c++)
        if (!p[i * planes + c]) return NeedleError_NullArgument;
    }
    Status s = gpu_convert_host(p, n, channels, format, o);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_convert_mono_host(const void *const *pcm, const size_t *num_values, const NeedleHipLaneFormat *formats,
                                              size_t num_streams, int16_t *const *out) {
  if (!pcm || !num_values || !formats || !out) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const void *> p;
    std::vector<size_t> n(num_values, num_values + num_streams);
    std::vector<int> channels(num_streams), fmts(num_streams);
    std::vector<int16_t *> o(out, out + num_streams);
    for (size_t i = 0; i < num_streams; i++) {  // every stream is checked before any pointer is counted off
      channels[i] = formats[i].channels;
      fmts[i] = formats[i].format;
      if (channels[i] < 1 || channels[i] > NEEDLE_HIP_MAX_CHANNELS || !sample_format_valid(fmts[i])) return NeedleError_InvalidArgument;
    }
    for (size_t i = 0; i < num_streams; i++) {
      const size_t planes = sample_format_planes(fmts[i], channels[i]);
      if (n[i] >= (size_t)channels[i]) {  // otherwise no whole frame: nothing is read or written
        if (!o[i]) return NeedleError_NullArgument;
        for (size_t c = 0; c < planes; c++)
          if (!pcm[p.size() + c]) return NeedleError_NullArgument;
      }
      p.insert(p.end(), pcm + p.size(), pcm + p.size() + planes);
    }
    Status s = gpu_convert_mono_host(p, n, channels, fmts, o);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_channel_mix_default(uint32_t channel_mask, NeedleHipChannelMix *out) {
  if (!out) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = channel_mix_default(channel_mask, out);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_rematrix_host(const void *const *pcm, const size_t *num_values, const NeedleHipLaneFormat *formats,
                                          const NeedleHipChannelMix *mixes, size_t num_streams, int16_t *const *out) {
  if (!pcm || !num_values || !formats || !mixes || !out) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const void *> p;
    std::vector<size_t> n(num_values, num_values + num_streams);
    std::vector<int> channels(num_streams), fmts(num_streams);
    std::vector<int16_t *> o(out, out + num_streams);
    for (size_t i = 0; i < num_streams; i++) {  // every stream and every mix is checked before any pointer is counted off
      channels[i] = formats[i].channels;
      fmts[i] = formats[i].format;
      if (channels[i] < 1 || channels[i] > NEEDLE_HIP_MAX_CHANNELS || !sample_format_valid(fmts[i])) return NeedleError_InvalidArgument;
      if (mixes[i].channels) {
        Status s = channel_mix_check(mixes[i], channels[i]);
        if (!s.ok()) return report(s);
      }
    }
    for (size_t i = 0; i < num_streams; i++) {
      const size_t planes = sample_format_planes(fmts[i], channels[i]);
      if (n[i] >= (size_t)channels[i]) {  // otherwise no whole frame: nothing is read or written
        if (!o[i]) return NeedleError_NullArgument;
        for (size_t c = 0; c < planes; c++)
          if (!pcm[p.size() + c]) return NeedleError_NullArgument;
      }
      p.insert(p.end(), pcm + p.size(), pcm + p.size() + planes);
    }
    Status s = gpu_convert_mono_host(p, n, channels, fmts, o, mixes);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

// ============================================================================================================
// search
// ============================================================================================================
enum NeedleError needle_hip_hamming_runs_device(const uint32_t *d_hashes, const NeedleHipSeq *seqs, size_t num_seqs,
                                                const NeedleHipProblem *problems, size_t num_problems,
                                                uint32_t threshold, NeedleHipRun *d_runs, uint32_t capacity,
                                                uint32_t *d_count, bool sync) {
  if (!d_hashes || !seqs || (!problems && num_problems) || !d_runs || !d_count) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = gpu_hamming_runs_device(d_hashes, seqs, num_seqs, problems, num_problems, threshold, d_runs, capacity,
                                       d_count, sync);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_hamming_runs_host(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *seqs,
                                              size_t num_seqs, const NeedleHipProblem *problems, size_t num_problems,
                                              uint32_t threshold, NeedleHipRun **runs, size_t *num_runs) {
  if ((!hashes && num_hashes) || !seqs || (!problems && num_problems) || !runs || !num_runs) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<NeedleHipRun> out;
    Status s = gpu_hamming_runs_host(hashes, num_hashes, seqs, num_seqs, problems, num_problems, threshold, &out);
    if (!s.ok()) return report(s);
    NeedleHipRun *arr = static_cast<NeedleHipRun *>(std::malloc(std::max<size_t>(out.size(), 1) * sizeof(NeedleHipRun)));
    if (!arr) return report(Status::Make(NeedleError_Unknown, "out of memory"));
    if (!out.empty()) std::memcpy(arr, out.data(), out.size() * sizeof(NeedleHipRun));
    *runs = arr;
    *num_runs = out.size();
    return NeedleError_Ok;
  });
}

// ============================================================================================================
// Streaming fingerprinter (feeder.hip)
// ============================================================================================================
enum NeedleError needle_hip_feeder_new(size_t lanes, int channels, int sample_rate, int format, uint32_t step,
                                       NeedleHipFeeder **output) {
  if (!output) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    auto f = std::make_unique<NeedleHipFeeder>();
    Status s = Feeder::Create(lanes, channels, sample_rate, format, step, &f->inner);
    if (!s.ok()) return report(s);
    *output = f.release();
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_feeder_new_lanes(const NeedleHipLaneFormat *formats, size_t lanes, uint32_t step, NeedleHipFeeder **output) {
  if (!output || !formats) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    auto f = std::make_unique<NeedleHipFeeder>();
    Status s = Feeder::CreateLanes(formats, lanes, step, &f->inner);
    if (!s.ok()) return report(s);
    *output = f.release();
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_feeder_lane_format(const NeedleHipFeeder *feeder, size_t lane, NeedleHipLaneFormat *format) {
  if (!feeder || !format) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = feeder->inner->LaneFormat(lane, format);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_feeder_reset_format(NeedleHipFeeder *feeder, const size_t *lanes, const NeedleHipLaneFormat *formats, size_t k) {
  if (!feeder || !lanes || !formats) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = feeder->inner->ResetFormat(lanes, formats, k);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_feeder_set_lane_mix(NeedleHipFeeder *feeder, const size_t *lanes, const NeedleHipChannelMix *mixes, size_t k) {
  if (!feeder || !lanes || !mixes) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = feeder->inner->SetLaneMix(lanes, mixes, k);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_feeder_switch_format(NeedleHipFeeder *feeder, const size_t *lanes, const NeedleHipLaneFormat *formats,
                                                 const NeedleHipChannelMix *mixes, size_t k) {
  if (!feeder || !lanes || !formats) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = feeder->inner->SwitchFormat(lanes, formats, mixes, k);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_feeder_lane_segments(const NeedleHipFeeder *feeder, size_t lane, NeedleHipSegment *out, size_t cap, size_t *count) {
  if (!feeder || !count || (cap && !out)) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = feeder->inner->LaneSegments(lane, out, cap, count);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

void needle_hip_feeder_free(NeedleHipFeeder *feeder) { delete feeder; }

enum NeedleError needle_hip_feeder_feed(NeedleHipFeeder *feeder, const void *const *pcm, const size_t *num_values) {
  if (!feeder || !pcm || !num_values) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = feeder->inner->Feed(pcm, num_values);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_feeder_finish(NeedleHipFeeder *feeder, const size_t *lanes, size_t k) {
  if (!feeder) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = feeder->inner->Finish(lanes, k);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_feeder_reset(NeedleHipFeeder *feeder, const size_t *lanes, size_t k) {
  if (!feeder) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = feeder->inner->Reset(lanes, k);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_feeder_ready(NeedleHipFeeder *feeder, size_t lane, size_t *kept_items,
                                         uint64_t *samples_per_channel_fed, bool *finished) {
  if (!feeder) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = feeder->inner->Ready(lane, kept_items, samples_per_channel_fed, finished);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_feeder_items(NeedleHipFeeder *feeder, size_t lane, size_t first, size_t count, uint32_t *items) {
  if (!feeder || (count && !items)) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = feeder->inner->Items(lane, first, count, items);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_feeder_frame_hashes(NeedleHipFeeder *feeder, size_t opening_lane, size_t ending_lane,
                                                uint64_t ending_seek_ns, float hash_duration, const char *md5, FrameHashes **output) {
  if (!feeder || !output) return NeedleError_NullArgument;
  if (!(hash_duration > 0.0f)) return NeedleError_AnalyzerInvalidHashDuration;
  return guarded([&]() -> NeedleError {
    bool ok = true;
    const ns_t hd = duration_from_secs_f32(hash_duration, &ok);
    uint32_t step = 0;
    if (!ok || !step_for_hash_duration(hd, &step)) return NeedleError_AnalyzerInvalidHashDuration;
    if (step != feeder->inner->step())
      return report(Status::Make(NeedleError_InvalidArgument, "feeder: hash_duration asks for another step than the feeder's"));
    const std::vector<uint32_t> *opening = nullptr, *ending = nullptr;
    Status s = feeder->inner->FinishedItems(opening_lane, &opening);
    if (s.ok() && ending_lane != SIZE_MAX) s = feeder->inner->FinishedItems(ending_lane, &ending);
    if (!s.ok()) return report(s);
    FrameHashesData d;
    attach_timestamps(opening->data(), opening->size(), step, false, 0, &d.opening);
    if (ending) attach_timestamps(ending->data(), ending->size(), step, true, ending_seek_ns, &d.ending);
    d.hash_duration = hd;
    d.md5 = md5 ? md5 : "";
    *output = new FrameHashes{std::move(d)};
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_feeder_state_bytes(const NeedleHipFeeder *feeder, uint64_t bytes[2]) {
  if (!feeder || !bytes) return NeedleError_NullArgument;
  feeder->inner->StateBytes(bytes);
  return NeedleError_Ok;
}

enum NeedleError needle_hip_feeder_set_audit(NeedleHipFeeder *feeder, bool on) {
  if (!feeder) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = feeder->inner->SetAudit(on);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_feeder_audit(NeedleHipFeeder *feeder, size_t lane, NeedleHipCertAudit *audit) {
  if (!feeder || !audit) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    uint64_t c[4] = {0, 0, 0, 0};
    NeedleHipCertAudit a{};
    Status s = feeder->inner->Audit(lane, c, &a.max_error_over_s, &a.max_s);
    if (!s.ok()) return report(s);
    a.items = c[0];
    a.accepted = c[1];
    a.accepted_mismatches = c[2];
    a.mismatches = c[3];
    *audit = a;
    return NeedleError_Ok;
  });
}

size_t needle_hip_feeder_num_ready(uint64_t samples_per_channel_fed, int sample_rate, int channels, uint32_t step, bool finished) {
  return feeder_num_ready(samples_per_channel_fed, sample_rate, channels, step, finished);
}

size_t needle_hip_feeder_num_ready_segments(const NeedleHipSegment *segments, size_t count, uint32_t step, bool finished) {
  return feeder_num_ready_segments(segments, count, step, finished);
}

// ============================================================================================================
// Streaming comparator (matcher.hip)
// ============================================================================================================
enum NeedleError needle_hip_matcher_new(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *sources,
                                        const uint32_t *min_len, size_t num_sources, size_t lanes, uint32_t threshold,
                                        NeedleHipMatcher **output) {
  if (!output || !sources || !min_len || (num_hashes && !hashes)) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    auto m = std::make_unique<NeedleHipMatcher>();
    Status s = Matcher::Create(hashes, num_hashes, sources, min_len, num_sources, lanes, threshold, &m->inner);
    if (!s.ok()) return report(s);
    *output = m.release();
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_matcher_new_regions(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *sources,
                                                const uint32_t *min_len, size_t num_sources, size_t regions, size_t lanes,
                                                uint32_t threshold, NeedleHipMatcher **output) {
  if (!output || !sources || !min_len || (num_hashes && !hashes)) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    auto m = std::make_unique<NeedleHipMatcher>();
    Status s = Matcher::CreateRegions(hashes, num_hashes, sources, min_len, num_sources, regions, lanes, threshold, &m->inner);
    if (!s.ok()) return report(s);
    *output = m.release();
    return NeedleError_Ok;
  });
}

void needle_hip_matcher_free(NeedleHipMatcher *matcher) { delete matcher; }

enum NeedleError needle_hip_matcher_feed(NeedleHipMatcher *matcher, const uint32_t *const *items, const size_t *num_items) {
  if (!matcher || !items || !num_items) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = matcher->inner->Feed(items, num_items);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_matcher_feed_from_feeder(NeedleHipMatcher *matcher, NeedleHipFeeder *feeder) {
  if (!matcher || !feeder) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = matcher->inner->FeedFromFeeder(feeder->inner.get());
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_matcher_finish(NeedleHipMatcher *matcher, const size_t *lanes, size_t k) {
  if (!matcher) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = matcher->inner->Finish(lanes, k);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_matcher_reset(NeedleHipMatcher *matcher, const size_t *lanes, size_t k) {
  if (!matcher) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = matcher->inner->Reset(lanes, k);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_matcher_ready(NeedleHipMatcher *matcher, size_t lane, size_t *num_runs, uint64_t *items_fed,
                                          bool *finished) {
  if (!matcher) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = matcher->inner->Ready(lane, num_runs, items_fed, finished);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_matcher_runs(NeedleHipMatcher *matcher, size_t lane, size_t first, size_t count, NeedleHipRun *runs) {
  if (!matcher || (count && !runs)) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = matcher->inner->Runs(lane, first, count, runs);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_matcher_open(NeedleHipMatcher *matcher, size_t lane, NeedleHipRun **runs, size_t *num_runs) {
  if (!matcher || !runs || !num_runs) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<NeedleHipRun> out;
    Status s = matcher->inner->Open(lane, &out);
    if (!s.ok()) return report(s);
    NeedleHipRun *buf = static_cast<NeedleHipRun *>(malloc(std::max<size_t>(out.size(), 1) * sizeof(NeedleHipRun)));
    if (!buf) return report(Status::Make(NeedleError_Unknown, "out of memory"));
    if (!out.empty()) memcpy(buf, out.data(), out.size() * sizeof(NeedleHipRun));
    *runs = buf;
    *num_runs = out.size();
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_matcher_stats(const NeedleHipMatcher *matcher, uint64_t stats[4]) {
  if (!matcher || !stats) return NeedleError_NullArgument;
  matcher->inner->Stats(stats);
  return NeedleError_Ok;
}

// ============================================================================================================
// Streaming all-pairs comparator (crossmatch.hip)
// ============================================================================================================
// The four ways in fill one spec (crossmatch.h): what a call does not take stays absent.
static CrossMatcher::Spec crossmatcher_spec(const NeedleHipSeq *resident, size_t num_resident, const uint32_t *resident_groups, size_t videos,
                                            const uint32_t *groups, size_t regions, const size_t *max_items, const uint32_t *min_len,
                                            uint32_t threshold) {
  CrossMatcher::Spec spec;
  spec.resident = resident;
  spec.residents = num_resident;
  spec.resident_groups = resident_groups;
  spec.arriving = videos;
  spec.groups = groups;
  spec.regions = regions;
  spec.max_items = max_items;
  spec.min_len = min_len;
  spec.threshold = threshold;
  return spec;
}

// ... and every way to a cross-matcher, the index's two included, wraps what `make` made.
static NeedleError crossmatcher_from(NeedleHipCrossMatcher **output, const std::function<Status(std::unique_ptr<CrossMatcher> *)> &make) {
  return guarded([&]() -> NeedleError {
    auto m = std::make_unique<NeedleHipCrossMatcher>();
    Status s = make(&m->inner);
    if (!s.ok()) return report(s);
    *output = m.release();
    return NeedleError_Ok;
  });
}
static NeedleError crossmatcher_new(const CrossMatcher::Spec &spec, const uint32_t *hashes, size_t num_hashes, NeedleHipCrossMatcher **output) {
  return crossmatcher_from(output, [&](std::unique_ptr<CrossMatcher> *out) { return CrossMatcher::Create(spec, hashes, num_hashes, false, out); });
}

enum NeedleError needle_hip_crossmatcher_new(size_t lanes, size_t max_items, uint32_t min_len, uint32_t threshold,
                                             NeedleHipCrossMatcher **output) {
  if (!output) return NeedleError_NullArgument;
  return crossmatcher_new(crossmatcher_spec(nullptr, 0, nullptr, lanes, nullptr, 1, &max_items, &min_len, threshold), nullptr, 0, output);
}

enum NeedleError needle_hip_crossmatcher_new_regions(size_t videos, size_t regions, const size_t *max_items, const uint32_t *min_len,
                                                     uint32_t threshold, NeedleHipCrossMatcher **output) {
  if (!output || !max_items || !min_len) return NeedleError_NullArgument;
  return crossmatcher_new(crossmatcher_spec(nullptr, 0, nullptr, videos, nullptr, regions, max_items, min_len, threshold), nullptr, 0, output);
}

enum NeedleError needle_hip_crossmatcher_new_resident(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *resident,
                                                      size_t num_resident, size_t videos, size_t regions, const size_t *max_items,
                                                      const uint32_t *min_len, uint32_t threshold, NeedleHipCrossMatcher **output) {
  if (!output || !max_items || !min_len || (num_resident && !resident) || (num_hashes && !hashes)) return NeedleError_NullArgument;
  return crossmatcher_new(crossmatcher_spec(resident, num_resident, nullptr, videos, nullptr, regions, max_items, min_len, threshold), hashes,
                          num_hashes, output);
}

enum NeedleError needle_hip_crossmatcher_new_grouped(const uint32_t *hashes, size_t num_hashes, const NeedleHipSeq *resident,
                                                     size_t num_resident, const uint32_t *resident_groups, size_t videos,
                                                     const uint32_t *groups, size_t regions, const size_t *max_items,
                                                     const uint32_t *min_len, uint32_t threshold, NeedleHipCrossMatcher **output) {
  if (!output || !max_items || !min_len || !groups || (num_resident && (!resident || !resident_groups)) || (num_hashes && !hashes))
    return NeedleError_NullArgument;
  return crossmatcher_new(crossmatcher_spec(resident, num_resident, resident_groups, videos, groups, regions, max_items, min_len, threshold),
                          hashes, num_hashes, output);
}

size_t needle_hip_crossmatcher_state_bytes_grouped(const NeedleHipSeq *resident, size_t num_resident, const uint32_t *resident_groups,
                                                   size_t videos, const uint32_t *groups, size_t regions, const size_t *max_items) {
  if (!groups) return 0;  // (without labels it would be another object's size)
  return CrossMatcher::StateBytes(crossmatcher_spec(resident, num_resident, resident_groups, videos, groups, regions, max_items, nullptr, 0));
}

enum NeedleError needle_hip_crossmatcher_groups(const NeedleHipCrossMatcher *matcher, uint32_t *labels, size_t n) {
  if (!matcher || !labels) return NeedleError_NullArgument;
  if (!matcher->inner->grouped())
    return report(Status::Make(NeedleError_InvalidArgument, "crossmatcher groups: not a grouped cross-matcher (needle_hip_crossmatcher_new_grouped makes one)"));
  const std::vector<uint32_t> &have = matcher->inner->labels();
  if (n < have.size()) return report(Status::Make(NeedleError_InvalidArgument, "crossmatcher groups: the array is shorter than the video list"));
  std::copy(have.begin(), have.end(), labels);
  return NeedleError_Ok;
}

void needle_hip_crossmatcher_free(NeedleHipCrossMatcher *matcher) { delete matcher; }

enum NeedleError needle_hip_crossmatcher_feed(NeedleHipCrossMatcher *matcher, const uint32_t *const *items, const size_t *num_items) {
  if (!matcher || !items || !num_items) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = matcher->inner->Feed(items, num_items);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_crossmatcher_feed_from_feeder(NeedleHipCrossMatcher *matcher, NeedleHipFeeder *feeder) {
  if (!matcher || !feeder) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = matcher->inner->FeedFromFeeder(feeder->inner.get());
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_crossmatcher_finish(NeedleHipCrossMatcher *matcher, const size_t *lanes, size_t k) {
  if (!matcher) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = matcher->inner->Finish(lanes, k);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_crossmatcher_ready(NeedleHipCrossMatcher *matcher, size_t *num_runs, bool *complete) {
  if (!matcher || !num_runs || !complete) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = matcher->inner->Ready(num_runs, complete);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_crossmatcher_lane(NeedleHipCrossMatcher *matcher, size_t lane, uint64_t *items_fed, bool *finished) {
  if (!matcher || !items_fed || !finished) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = matcher->inner->Lane(lane, items_fed, finished);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_crossmatcher_runs(NeedleHipCrossMatcher *matcher, size_t first, size_t count, NeedleHipRun *runs) {
  if (!matcher || (count && !runs)) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = matcher->inner->Runs(first, count, runs);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_crossmatcher_stats(const NeedleHipCrossMatcher *matcher, uint64_t stats[4]) {
  if (!matcher || !stats) return NeedleError_NullArgument;
  matcher->inner->Stats(stats);
  return NeedleError_Ok;
}

size_t needle_hip_crossmatcher_state_bytes(size_t lanes, size_t max_items) { return needle_hip_crossmatcher_state_bytes_regions(lanes, 1, &max_items); }

size_t needle_hip_crossmatcher_state_bytes_regions(size_t videos, size_t regions, const size_t *max_items) {
  return needle_hip_crossmatcher_state_bytes_resident(nullptr, 0, videos, regions, max_items);
}

size_t needle_hip_crossmatcher_state_bytes_resident(const NeedleHipSeq *resident, size_t num_resident, size_t videos, size_t regions,
                                                    const size_t *max_items) {
  return CrossMatcher::StateBytes(crossmatcher_spec(resident, num_resident, nullptr, videos, nullptr, regions, max_items, nullptr, 0));
}

enum NeedleError needle_hip_crossmatcher_resident(const NeedleHipCrossMatcher *matcher, size_t *num_resident) {
  if (!matcher || !num_resident) return NeedleError_NullArgument;
  *num_resident = matcher->inner->residents();
  return NeedleError_Ok;
}

enum NeedleError needle_hip_crossmatcher_shape(const NeedleHipCrossMatcher *matcher, size_t *videos, size_t *regions) {
  if (!matcher || !videos || !regions) return NeedleError_NullArgument;
  *videos = matcher->inner->videos();
  *regions = matcher->inner->regions();
  return NeedleError_Ok;
}

// ============================================================================================================
// FrameHashes
// ============================================================================================================
enum NeedleError needle_hip_frame_hashes_new(const uint32_t *opening_hashes, const uint64_t *opening_ts_ns,
                                             size_t num_opening, const uint32_t *ending_hashes,
                                             const uint64_t *ending_ts_ns, size_t num_ending,
                                             uint64_t hash_duration_ns, const char *md5, FrameHashes **output) {
  if (!output || (num_opening && (!opening_hashes || !opening_ts_ns)) || (num_ending && (!ending_hashes || !ending_ts_ns)))
    return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    auto *fh = new FrameHashes();
    fh->d.opening.resize(num_opening);
    for (size_t i = 0; i < num_opening; i++) fh->d.opening[i] = HashTs{opening_hashes[i], opening_ts_ns[i]};
    fh->d.ending.resize(num_ending);
    for (size_t i = 0; i < num_ending; i++) fh->d.ending[i] = HashTs{ending_hashes[i], ending_ts_ns[i]};
    fh->d.hash_duration = hash_duration_ns;
    fh->d.md5 = md5 ? md5 : "";
    *output = fh;
    return NeedleError_Ok;
  });
}

void needle_hip_frame_hashes_free(FrameHashes *frame_hashes) { delete frame_hashes; }

size_t needle_hip_frame_hashes_len(const FrameHashes *fh, bool ending) {
  return !fh ? 0 : (ending ? fh->d.ending.size() : fh->d.opening.size());
}

enum NeedleError needle_hip_frame_hashes_copy(const FrameHashes *fh, bool ending, uint32_t *hashes, uint64_t *ts_ns,
                                              size_t capacity) {
  if (!fh) return NeedleError_NullArgument;
  const std::vector<HashTs> &v = ending ? fh->d.ending : fh->d.opening;
  if (capacity < v.size()) return NeedleError_InvalidArgument;
  for (size_t i = 0; i < v.size(); i++) {
    if (hashes) hashes[i] = v[i].hash;
    if (ts_ns) ts_ns[i] = v[i].ts;
  }
  return NeedleError_Ok;
}

uint64_t needle_hip_frame_hashes_hash_duration_ns(const FrameHashes *fh) { return fh ? fh->d.hash_duration : 0; }
const char *needle_hip_frame_hashes_md5(const FrameHashes *fh) { return fh ? fh->d.md5.c_str() : ""; }

enum NeedleError needle_hip_frame_hashes_read(const char *path, FrameHashes **output) {
  if (!path || !output) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    auto fh = new FrameHashes();
    Status s = frame_hashes_read(path, &fh->d);
    if (!s.ok()) {
      delete fh;
      return report(s);
    }
    *output = fh;
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_frame_hashes_write(const FrameHashes *fh, const char *path) {
  if (!fh || !path) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = frame_hashes_write(path, fh->d);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_header_md5(const char *path, char out[33]) {
  if (!path || !out) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::string md5;
    Status s = header_md5(path, &md5);
    if (!s.ok()) return report(s);
    std::memcpy(out, md5.c_str(), 33);
    return NeedleError_Ok;
  });
}

// ============================================================================================================
// Analyzer / Comparator in memory
// ============================================================================================================
enum NeedleError needle_hip_analyzer_run_pcm(struct NeedleAudioAnalyzer *analyzer, const int16_t *const *pcm,
                                             const size_t *num_values, int channels, int sample_rate,
                                             float hash_duration, bool persist) {
  if (!analyzer || !pcm || !num_values) return NeedleError_NullArgument;
  if (!(hash_duration > 0.0f)) return NeedleError_AnalyzerInvalidHashDuration;
  return guarded([&]() -> NeedleError {
    bool ok = true;
    const ns_t hd = duration_from_secs_f32(hash_duration, &ok);
    if (!ok) return NeedleError_AnalyzerInvalidHashDuration;
    const size_t n = analyzer->inner.videos().size();
    std::vector<PcmView> views(n);
    for (size_t i = 0; i < n; i++) {
      if (!pcm[i] && num_values[i]) return NeedleError_NullArgument;
      views[i] = PcmView{pcm[i], num_values[i]};
    }
    std::vector<FrameHashesData> out;
    Status s = analyzer->inner.run_pcm(views, channels, sample_rate, hd, persist, &out);
    if (!s.ok()) return report(s);
    analyzer->frame_hashes.clear();
    for (FrameHashesData &d : out) analyzer->frame_hashes.push_back(FrameHashes{std::move(d)});
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_analyzer_run_pcm_format(struct NeedleAudioAnalyzer *analyzer, const void *const *pcm,
                                                    const size_t *num_values, int channels, int sample_rate, int format,
                                                    float hash_duration, bool persist) {
  if (!analyzer || !pcm || !num_values) return NeedleError_NullArgument;
  if (!(hash_duration > 0.0f)) return NeedleError_AnalyzerInvalidHashDuration;
  if (!sample_format_valid(format)) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    bool ok = true;
    const ns_t hd = duration_from_secs_f32(hash_duration, &ok);
    if (!ok) return NeedleError_AnalyzerInvalidHashDuration;
    if (channels < 1 || channels > NEEDLE_HIP_MAX_CHANNELS)
      return report(Status::Make(NeedleError_InvalidArgument, "channels must be 1 to " + std::to_string(NEEDLE_HIP_MAX_CHANNELS)));
    const size_t n = analyzer->inner.videos().size(), planes = sample_format_planes(format, channels);
    std::vector<const void *> p(pcm, pcm + n * planes);
    std::vector<size_t> lens(num_values, num_values + n);
    for (size_t i = 0; i < n * planes; i++)
      if (!p[i] && lens[i / planes]) return NeedleError_NullArgument;
    std::vector<FrameHashesData> out;
    Status s = analyzer->inner.run_pcm_format(p, lens, channels, sample_rate, format, hd, persist, &out);
    if (!s.ok()) return report(s);
    analyzer->frame_hashes.clear();
    for (FrameHashesData &d : out) analyzer->frame_hashes.push_back(FrameHashes{std::move(d)});
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_analyzer_run_pcm_formats(struct NeedleAudioAnalyzer *analyzer, const void *const *pcm,
                                                     const size_t *num_values, const NeedleHipLaneFormat *formats,
                                                     const NeedleHipChannelMix *mixes, float hash_duration, bool persist) {
  if (!analyzer || !pcm || !num_values || !formats) return NeedleError_NullArgument;
  if (!(hash_duration > 0.0f)) return NeedleError_AnalyzerInvalidHashDuration;
  return guarded([&]() -> NeedleError {
    bool ok = true;
    const ns_t hd = duration_from_secs_f32(hash_duration, &ok);
    if (!ok) return NeedleError_AnalyzerInvalidHashDuration;
    const size_t n = analyzer->inner.videos().size();
    size_t planes = 0;
    for (size_t i = 0; i < n; i++) {
      // (the planes of a stream cannot be counted without these two; run_pcm_formats checks the rest)
      if (!sample_format_valid(formats[i].format) || formats[i].channels < 1 || formats[i].channels > NEEDLE_HIP_MAX_CHANNELS)
        return report(Status::Make(NeedleError_InvalidArgument, "stream " + std::to_string(i) + ": unknown sample format or channel count"));
      for (size_t c = 0; c < sample_format_planes(formats[i].format, formats[i].channels); c++)
        if (!pcm[planes++] && num_values[i]) return NeedleError_NullArgument;
    }
    std::vector<const void *> p(pcm, pcm + planes);
    std::vector<size_t> lens(num_values, num_values + n);
    std::vector<FrameHashesData> out;
    Status s = analyzer->inner.run_pcm_formats(p, lens, formats, mixes, hd, persist, &out);
    if (!s.ok()) return report(s);
    analyzer->frame_hashes.clear();
    for (FrameHashesData &d : out) analyzer->frame_hashes.push_back(FrameHashes{std::move(d)});
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_analyzer_set_channel_mix(struct NeedleAudioAnalyzer *analyzer, const NeedleHipChannelMix *mix) {
  if (!analyzer) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    if (mix) {
      Status s = channel_mix_check(*mix, mix->channels);
      if (!s.ok()) return report(s);
    }
    analyzer->inner.with_channel_mix(mix);
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_analyzer_set_layout_downmix(struct NeedleAudioAnalyzer *analyzer, bool on) {
  if (!analyzer) return NeedleError_NullArgument;
  analyzer->inner.with_layout_downmix(on);
  return NeedleError_Ok;
}

enum NeedleError needle_hip_comparator_set_layout_downmix(struct NeedleAudioComparator *comparator, bool on) {
  if (!comparator) return NeedleError_NullArgument;
  comparator->inner.with_layout_downmix(on);
  return NeedleError_Ok;
}

enum NeedleError needle_hip_comparator_run_with_frame_hashes(const struct NeedleAudioComparator *comparator,
                                                             const FrameHashes *const *frame_hashes,
                                                             size_t num_videos, bool display, bool use_skip_files,
                                                             bool write_skip_files, NeedleHipSearchResult *results) {
  if (!comparator || !frame_hashes || !results) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const FrameHashesData *> fh(num_videos);
    for (size_t i = 0; i < num_videos; i++) {
      if (!frame_hashes[i]) return NeedleError_NullArgument;
      fh[i] = &frame_hashes[i]->d;
    }
    std::vector<VideoResult> res;
    Status s = comparator->inner.run_with_frame_hashes(fh, display, use_skip_files, write_skip_files, true, &res);
    if (!s.ok()) return report(s);
    for (size_t i = 0; i < num_videos; i++) fill_result(res[i], &results[i]);
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_comparator_results_from_runs(const struct NeedleAudioComparator *comparator,
                                                         const FrameHashes *const *frame_hashes, size_t num_videos,
                                                         const NeedleHipRun *runs, size_t num_runs, size_t first_video,
                                                         size_t video_count, NeedleHipSearchResult *results) {
  if (!comparator || !frame_hashes || !results || (!runs && num_runs)) return NeedleError_NullArgument;
  if (first_video > num_videos || video_count > num_videos - first_video) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const FrameHashesData *> fh(num_videos);
    for (size_t i = 0; i < num_videos; i++) {
      if (!frame_hashes[i]) return NeedleError_NullArgument;
      fh[i] = &frame_hashes[i]->d;
    }
    std::vector<VideoResult> res;
    Status s = comparator->inner.results_from_runs(fh, runs, num_runs, false, false, false, &res, first_video,
                                                   first_video + video_count);
    if (!s.ok()) return report(s);
    for (size_t i = 0; i < num_videos; i++) fill_result(res[i], &results[i]);
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_comparator_results_from_runs_evidence(const struct NeedleAudioComparator *comparator,
                                                                  const FrameHashes *const *frame_hashes, size_t num_videos,
                                                                  const NeedleHipRun *runs, size_t num_runs, size_t first_video,
                                                                  size_t video_count, NeedleHipSearchResult *results,
                                                                  NeedleHipSearchEvidence *evidence) {
  if (!comparator || !frame_hashes || !evidence || (!runs && num_runs)) return NeedleError_NullArgument;
  if (first_video > num_videos || video_count > num_videos - first_video) return NeedleError_InvalidArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const FrameHashesData *> fh(num_videos);
    for (size_t i = 0; i < num_videos; i++) {
      if (!frame_hashes[i]) return NeedleError_NullArgument;
      fh[i] = &frame_hashes[i]->d;
    }
    std::vector<VideoResult> res;
    std::vector<NeedleHipSearchEvidence> ev;
    Status s = comparator->inner.results_from_runs(fh, runs, num_runs, false, false, false, &res, first_video,
                                                   first_video + video_count, &ev);
    if (!s.ok()) return report(s);
    for (size_t i = 0; i < num_videos; i++) {
      if (results) fill_result(res[i], &results[i]);
      evidence[i] = ev[i];
    }
    return NeedleError_Ok;
  });
}

// ---- groups of videos (needle_hip.h "A library of many shows") ----
enum NeedleError needle_hip_group_pairs(const uint32_t *groups, size_t num_videos, uint32_t *pair_videos, size_t capacity,
                                        uint64_t *num_pairs) {
  if (!num_pairs || (!groups && num_videos)) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    if (num_videos > UINT32_MAX) return report(Status::Make(NeedleError_InvalidArgument, "group_pairs: more than 2^32 videos"));
    const GroupTables tables(groups, num_videos);
    *num_pairs = tables.pairs();
    if (pair_videos) {
      const GroupView view = tables.view();
      for (uint64_t p = 0; p < std::min<uint64_t>(capacity, tables.pairs()); p++)
        (void)grouped_pair_at(view, p, &pair_videos[2 * p], &pair_videos[2 * p + 1]);
    }
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_comparator_run_with_frame_hashes_grouped(const struct NeedleAudioComparator *comparator,
                                                                     const FrameHashes *const *frame_hashes, size_t num_videos,
                                                                     const uint32_t *groups, bool display, bool use_skip_files,
                                                                     bool write_skip_files, NeedleHipSearchResult *results) {
  if (!comparator || !frame_hashes || !results) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const FrameHashesData *> fh(num_videos);
    for (size_t i = 0; i < num_videos; i++) {
      if (!frame_hashes[i]) return NeedleError_NullArgument;
      fh[i] = &frame_hashes[i]->d;
    }
    std::vector<VideoResult> res;
    Status s = comparator->inner.run_with_frame_hashes(fh, display, use_skip_files, write_skip_files, true, &res, groups);
    if (!s.ok()) return report(s);
    for (size_t i = 0; i < num_videos; i++) fill_result(res[i], &results[i]);
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_comparator_results_from_runs_grouped(const struct NeedleAudioComparator *comparator,
                                                                 const FrameHashes *const *frame_hashes, size_t num_videos,
                                                                 const uint32_t *groups, const NeedleHipRun *runs, size_t num_runs,
                                                                 NeedleHipSearchResult *results) {
  if (!comparator || !frame_hashes || !results || (!runs && num_runs)) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const FrameHashesData *> fh(num_videos);
    for (size_t i = 0; i < num_videos; i++) {
      if (!frame_hashes[i]) return NeedleError_NullArgument;
      fh[i] = &frame_hashes[i]->d;
    }
    std::unique_ptr<const GroupTables> tables(groups ? new GroupTables(groups, num_videos) : nullptr);
    if (tables) {
      const uint64_t buckets = tables->pairs() * (comparator->inner.include_endings() ? 2 : 1);
      if (buckets > UINT32_MAX)
        return report(Status::Make(NeedleError_InvalidArgument, "library too large for one search call: more than 2^32 hashes or sequence pairs"));
      if (comparator->inner.include_endings())
        for (size_t v = 0; v < num_videos; v++)
          if (fh[v]->ending.empty() && tables->size[tables->group_of[v]] > 1)
            return report(Status::Make(NeedleError_Unknown, "no ending hash data present"));
      for (size_t q = 0; q < num_runs; q++)
        if (runs[q].problem >= buckets)
          return report(Status::Make(NeedleError_InvalidArgument, "results_from_runs_grouped: run " + std::to_string(q) + " names problem " +
                                                                      std::to_string(runs[q].problem) + ", the groups have " +
                                                                      std::to_string(buckets) + " (a run list in another numbering?)"));
    }
    std::vector<VideoResult> res;
    Status s = comparator->inner.results_from_runs(fh, runs, num_runs, false, false, false, &res, 0, ~(size_t)0, nullptr, tables.get());
    if (!s.ok()) return report(s);
    for (size_t i = 0; i < num_videos; i++) fill_result(res[i], &results[i]);
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_comparator_run_grouped(const struct NeedleAudioComparator *comparator, const uint32_t *groups,
                                                   size_t num_groups_entries, bool analyze, bool display, bool use_skip_files,
                                                   bool write_skip_files) {
  if (!comparator) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    if (groups && num_groups_entries != comparator->inner.videos().size())
      return report(Status::Make(NeedleError_InvalidArgument, "run_grouped: " + std::to_string(num_groups_entries) + " group labels for " +
                                                                  std::to_string(comparator->inner.videos().size()) + " videos"));
    std::vector<VideoResult> res;
    Status s = comparator->inner.run(analyze, display, use_skip_files, write_skip_files, true, &res, groups);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_index_new(const struct NeedleAudioComparator *comparator, NeedleHipIndex **output) {
  if (!comparator || !output) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    NeedleHipIndex *index = new NeedleHipIndex(comparator->inner);
    Status s = index->inner.init();
    if (!s.ok()) {
      delete index;
      return report(s);
    }
    *output = index;
    return NeedleError_Ok;
  });
}

void needle_hip_index_free(NeedleHipIndex *index) {
  if (!index) return;
  guarded([&]() -> NeedleError {
    delete index;
    return NeedleError_Ok;
  });
}

size_t needle_hip_index_len(const NeedleHipIndex *index) { return index ? index->inner.size() : 0; }

enum NeedleError needle_hip_index_add(NeedleHipIndex *index, const FrameHashes *const *frame_hashes, size_t k) {
  if (!index) return NeedleError_NullArgument;
  if (k == 0) return report(Status::Make(NeedleError_InvalidArgument, "index add: no videos"));
  if (!frame_hashes) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const FrameHashesData *> fh(k);
    for (size_t i = 0; i < k; i++) {
      if (!frame_hashes[i]) return NeedleError_NullArgument;
      fh[i] = &frame_hashes[i]->d;
    }
    Status s = index->inner.add(fh);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_index_results(const NeedleHipIndex *index, NeedleHipSearchResult *results, size_t n) {
  if (!index) return NeedleError_NullArgument;
  const std::vector<NeedleHipSearchResult> &have = index->inner.results();
  if (n < have.size()) return report(Status::Make(NeedleError_InvalidArgument, "index results: buffer shorter than the index"));
  if (!results && !have.empty()) return NeedleError_NullArgument;
  if (!have.empty()) std::memcpy(results, have.data(), have.size() * sizeof(NeedleHipSearchResult));
  return NeedleError_Ok;
}

enum NeedleError needle_hip_index_evidence(const NeedleHipIndex *index, NeedleHipSearchEvidence *evidence, size_t n) {
  if (!index) return NeedleError_NullArgument;
  const size_t have = index->inner.size();
  if (n < have) return report(Status::Make(NeedleError_InvalidArgument, "index evidence: buffer shorter than the index"));
  if (!evidence && have) return NeedleError_NullArgument;
  if (!have) return NeedleError_Ok;
  return guarded([&]() -> NeedleError {
    Status s = index->inner.evidence(evidence);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_index_pairs_searched(const NeedleHipIndex *index, uint64_t *total, uint64_t *last) {
  if (!index) return NeedleError_NullArgument;
  if (total) *total = index->inner.pairs_total();
  if (last) *last = index->inner.pairs_last();
  return NeedleError_Ok;
}

enum NeedleError needle_hip_index_pairs_scanned(const NeedleHipIndex *index, uint64_t *total, uint64_t *last) {
  if (!index) return NeedleError_NullArgument;
  if (total) *total = index->inner.scanned_total();
  if (last) *last = index->inner.scanned_last();
  return NeedleError_Ok;
}

enum NeedleError needle_hip_index_crossmatcher_new(NeedleHipIndex *index, size_t videos, const size_t *max_items, const uint32_t *min_len,
                                                   NeedleHipCrossMatcher **output) {
  if (!index || !max_items || !min_len || !output) return NeedleError_NullArgument;
  return crossmatcher_from(output, [&](std::unique_ptr<CrossMatcher> *out) { return index->inner.crossmatcher(videos, max_items, min_len, out); });
}

enum NeedleError needle_hip_index_add_matched(NeedleHipIndex *index, NeedleHipCrossMatcher *matcher, const FrameHashes *const *frame_hashes,
                                              size_t k) {
  if (!index || !matcher) return NeedleError_NullArgument;
  if (k == 0) return report(Status::Make(NeedleError_InvalidArgument, "index add: no videos"));
  if (!frame_hashes) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const FrameHashesData *> fh(k);
    for (size_t i = 0; i < k; i++) {
      if (!frame_hashes[i]) return NeedleError_NullArgument;
      fh[i] = &frame_hashes[i]->d;
    }
    Status s = index->inner.add_matched(matcher->inner.get(), fh);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_index_crossmatcher_new_grouped(NeedleHipIndex *index, size_t videos, const uint32_t *groups, const size_t *max_items,
                                                           const uint32_t *min_len, NeedleHipCrossMatcher **output) {
  if (!index || !groups || !max_items || !min_len || !output) return NeedleError_NullArgument;
  return crossmatcher_from(output, [&](std::unique_ptr<CrossMatcher> *out) {
    return index->inner.crossmatcher_grouped(videos, groups, max_items, min_len, out);
  });
}

enum NeedleError needle_hip_index_add_matched_grouped(NeedleHipIndex *index, NeedleHipCrossMatcher *matcher,
                                                      const FrameHashes *const *frame_hashes, size_t k) {
  if (!index || !matcher) return NeedleError_NullArgument;
  if (k == 0) return report(Status::Make(NeedleError_InvalidArgument, "index add: no videos"));
  if (!frame_hashes) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const FrameHashesData *> fh(k);
    for (size_t i = 0; i < k; i++) {
      if (!frame_hashes[i]) return NeedleError_NullArgument;
      fh[i] = &frame_hashes[i]->d;
    }
    Status s = index->inner.add_matched_grouped(matcher->inner.get(), fh);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_index_matcher_new(NeedleHipIndex *index, size_t videos, NeedleHipMatcher **output) {
  if (!index || !output) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    auto m = std::make_unique<NeedleHipMatcher>();
    Status s = index->inner.matcher(videos, &m->inner);
    if (!s.ok()) return report(s);
    *output = m.release();
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_index_add_streamed(NeedleHipIndex *index, NeedleHipMatcher *matcher, NeedleHipCrossMatcher *crossmatcher,
                                               const FrameHashes *const *frame_hashes, size_t k) {
  if (!index || !matcher) return NeedleError_NullArgument;
  if (k == 0) return report(Status::Make(NeedleError_InvalidArgument, "index add: no videos"));
  if (!frame_hashes) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const FrameHashesData *> fh(k);
    for (size_t i = 0; i < k; i++) {
      if (!frame_hashes[i]) return NeedleError_NullArgument;
      fh[i] = &frame_hashes[i]->d;
    }
    Status s = index->inner.add_streamed(matcher->inner.get(), crossmatcher ? crossmatcher->inner.get() : nullptr, fh);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_index_remove(NeedleHipIndex *index, const size_t *positions, size_t k) {
  if (!index || !positions) return NeedleError_NullArgument;
  if (k == 0) return report(Status::Make(NeedleError_InvalidArgument, "index remove: no positions"));
  return guarded([&]() -> NeedleError {
    Status s = index->inner.remove(std::vector<size_t>(positions, positions + k));
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_index_replace(NeedleHipIndex *index, const size_t *positions, const FrameHashes *const *frame_hashes, size_t k) {
  if (!index || !positions || !frame_hashes) return NeedleError_NullArgument;
  if (k == 0) return report(Status::Make(NeedleError_InvalidArgument, "index replace: no positions"));
  return guarded([&]() -> NeedleError {
    std::vector<const FrameHashesData *> fh(k);
    for (size_t i = 0; i < k; i++) {
      if (!frame_hashes[i]) return NeedleError_NullArgument;
      fh[i] = &frame_hashes[i]->d;
    }
    Status s = index->inner.replace(std::vector<size_t>(positions, positions + k), fh);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_index_store_sizes(const NeedleHipIndex *index, uint64_t sizes[4]) {
  if (!index || !sizes) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    Status s = index->inner.store_sizes(sizes);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

// ---- a grouped index (needle_hip.h "A grouped index") ----
enum NeedleError needle_hip_index_new_grouped(const struct NeedleAudioComparator *comparator, NeedleHipIndex **output) {
  if (!comparator || !output) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    NeedleHipIndex *index = new NeedleHipIndex(comparator->inner, true);
    Status s = index->inner.init();
    if (!s.ok()) {
      delete index;
      return report(s);
    }
    *output = index;
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_index_add_grouped(NeedleHipIndex *index, const FrameHashes *const *frame_hashes, const uint32_t *groups,
                                              size_t k) {
  if (!index) return NeedleError_NullArgument;
  if (k == 0) return report(Status::Make(NeedleError_InvalidArgument, "index add: no videos"));
  if (!frame_hashes || !groups) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<const FrameHashesData *> fh(k);
    for (size_t i = 0; i < k; i++) {
      if (!frame_hashes[i]) return NeedleError_NullArgument;
      fh[i] = &frame_hashes[i]->d;
    }
    Status s = index->inner.add_grouped(fh, groups);
    return s.ok() ? NeedleError_Ok : report(s);
  });
}

enum NeedleError needle_hip_index_groups(const NeedleHipIndex *index, uint32_t *labels, size_t n) {
  if (!index) return NeedleError_NullArgument;
  if (!index->inner.grouped()) return report(Status::Make(NeedleError_InvalidArgument, "index groups: not a grouped index"));
  const std::vector<uint32_t> &have = index->inner.labels();
  if (n < have.size()) return report(Status::Make(NeedleError_InvalidArgument, "index groups: buffer shorter than the index"));
  if (!labels && !have.empty()) return NeedleError_NullArgument;
  if (!have.empty()) std::memcpy(labels, have.data(), have.size() * sizeof(uint32_t));
  return NeedleError_Ok;
}

// ============================================================================================================
// Compressed fingerprints (fp_codec.hip)
// ============================================================================================================
extern "C++" {
namespace {
template <class T>
T *malloc_copy(const T *src, size_t n, size_t extra = 0) {
  T *arr = static_cast<T *>(std::malloc(std::max<size_t>(n + extra, 1) * sizeof(T)));
  if (arr && n) std::memcpy(arr, src, n * sizeof(T));
  return arr;
}
}  // namespace
}  // extern "C++"

size_t needle_hip_fingerprint_compressed_bound(size_t items) { return (size_t)fpc_compressed_bound(items); }

enum NeedleError needle_hip_fingerprint_compress_host(const uint32_t *items, const uint64_t *item_offsets, size_t count, int algorithm,
                                                      uint8_t **blobs, uint64_t *blob_offsets) {
  if (!item_offsets || !blobs || !blob_offsets || (!items && item_offsets[count] > item_offsets[0])) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<uint8_t> out;
    std::vector<uint64_t> off;
    Status s = gpu_fp_compress_host(items, item_offsets, count, algorithm, &out, &off);
    if (!s.ok()) return report(s);
    uint8_t *arr = malloc_copy(out.data(), out.size());
    if (!arr) return report(Status::Make(NeedleError_Unknown, "out of memory"));
    *blobs = arr;
    std::memcpy(blob_offsets, off.data(), (count + 1) * sizeof(uint64_t));
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_fingerprint_decompress_host(const uint8_t *blobs, const uint64_t *blob_offsets, size_t count, uint32_t **items,
                                                        uint64_t *item_offsets, int32_t *algorithms, int32_t *status) {
  if (!blob_offsets || !items || !item_offsets || (count && (!algorithms || !status)) || (!blobs && blob_offsets[count] > blob_offsets[0]))
    return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<uint32_t> out;
    std::vector<uint64_t> off;
    std::vector<int32_t> alg, st;
    Status s = gpu_fp_decompress_host(blobs, blob_offsets, count, &out, &off, &alg, &st);
    if (!s.ok()) return report(s);
    uint32_t *arr = malloc_copy(out.data(), out.size());
    if (!arr) return report(Status::Make(NeedleError_Unknown, "out of memory"));
    *items = arr;
    std::memcpy(item_offsets, off.data(), (count + 1) * sizeof(uint64_t));
    if (count) {
      std::memcpy(algorithms, alg.data(), count * sizeof(int32_t));
      std::memcpy(status, st.data(), count * sizeof(int32_t));
    }
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_feeder_compressed(NeedleHipFeeder *feeder, size_t lane, int algorithm, uint8_t **blob, size_t *size) {
  if (!feeder || !blob || !size) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    const std::vector<uint32_t> *kept = nullptr;
    Status s = feeder->inner->FinishedItems(lane, &kept);
    if (!s.ok()) return report(s);
    const uint64_t item_off[2] = {0, kept->size()};
    std::vector<uint8_t> out;
    std::vector<uint64_t> off;
    if (!(s = gpu_fp_compress_host(kept->data(), item_off, 1, algorithm, &out, &off)).ok()) return report(s);
    uint8_t *arr = malloc_copy(out.data(), out.size());
    if (!arr) return report(Status::Make(NeedleError_Unknown, "out of memory"));
    *blob = arr;
    *size = out.size();
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_fingerprint_base64_encode(const uint8_t *data, size_t size, char **text, size_t *text_size) {
  if ((!data && size) || !text || !text_size) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    const std::string out = fp_base64_encode(data, size);
    char *arr = malloc_copy(out.data(), out.size(), 1);
    if (!arr) return report(Status::Make(NeedleError_Unknown, "out of memory"));
    arr[out.size()] = 0;
    *text = arr;
    *text_size = out.size();
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_fingerprint_base64_decode(const char *text, size_t text_size, uint8_t **data, size_t *size) {
  if ((!text && text_size) || !data || !size) return NeedleError_NullArgument;
  return guarded([&]() -> NeedleError {
    std::vector<uint8_t> out;
    if (!fp_base64_decode(text, text_size, &out))
      return report(Status::Make(NeedleError_InvalidArgument, "base64: a character outside the URL-safe alphabet, or a length of 1 mod 4"));
    uint8_t *arr = malloc_copy(out.data(), out.size());
    if (!arr) return report(Status::Make(NeedleError_Unknown, "out of memory"));
    *data = arr;
    *size = out.size();
    return NeedleError_Ok;
  });
}

enum NeedleError needle_hip_fingerprint_codec_tiles(size_t *compress_items, size_t *decompress_symbols) {
  if (!compress_items || !decompress_symbols) return NeedleError_NullArgument;
  *compress_items = kFpcTileItems;
  *decompress_symbols = kFpdTileSymbols;
  return NeedleError_Ok;
}

enum NeedleError needle_hip_fingerprint_simhash(const uint32_t *items, size_t count, uint32_t *hash) {
  if ((!items && count) || !hash) return NeedleError_NullArgument;
  *hash = simhash32(items, count);
  return NeedleError_Ok;
}

}  // extern "C"

// library.cpp needs these two without seeing the handle layouts twice
namespace needle {
const Comparator &comparator_of(const NeedleAudioComparator *c) { return c->inner; }
FrameHashes *make_frame_hashes(FrameHashesData &&d) { return new FrameHashes{std::move(d)}; }
void fill_c_result(const VideoResult &v, NeedleHipSearchResult *r) { fill_result(v, r); }
}  // namespace needle
