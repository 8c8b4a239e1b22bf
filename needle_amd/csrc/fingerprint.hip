// GPU fingerprinter: the chromaprint Context replacement behind
// needle/src/audio/analyzer.rs:176-300 (start/feed/finish/get_fingerprint_raw), batched over streams.
//
//   stft_chroma       : s16 PCM -> Hamming window -> two real frames per 4096-pt complex FFT (f64, in place in
//                       LDS) -> |X|^2 over bins 10..1307 -> 12 pitch-class energies per frame   [frames][12] f64
//   features_classify : temporal FIR + L2 normalise + 16 classifiers -> u32 per kept item (classify_kernels.h)
//
// HBM traffic that matters is the PCM read (2 B/sample, each sample touched by 3 overlapping frames:
// re-reads are served by L2) and 96 B/frame of chroma; everything else stays on chip.
//
// This unit holds the constant tables, the workspaces and the three drivers of those kernels: the one-shot
// gpu_fingerprint_device, the streaming feeder's gpu_fingerprint_feed_device and gpu_fingerprint_audit_device.  The
// kernels are in classify_kernels.h, stft_kernel.h and stft32_kernel.h (the latter compiled in fingerprint32.hip), the
// host-upload planner in fingerprint_host.hip.  The drivers share
//   plan_chunk (and plan_feed beside it) : spans -> one chunk's FpStream table and its totals; every FpStream field
//                       convention is there;
//   enqueue_certified : stft_chroma32 -> features_cert -> stft_chroma<LISTED> -> fixup_items, from a CertChain;
//   enqueue_f64       : stft_chroma -> features_classify, from an F64Chain;
// and every kernel is launched from exactly one place.  Where the drivers differ is a field of those blocks: the tables
// of the first pass and of the tail (one table, or a feed's `first` and `second`), PHASED tiles, where the
// recomputation writes, the first pass's schedule, the recomputation's grid and variant, the pipe's stream and events,
// the control block's zeroed words, what is counted, and whether a launch is timed.
#include "classify_kernels.h"
#include "fingerprint32.h"
#include "hipctx.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>

namespace needle {

using core::cd;

namespace {

// ---- constant tables, generated on the host in double and uploaded once per device --------------------
struct FpTables {
  cd *tw = nullptr;                 // [4096] e^{-2 pi i k/4096}
  uint16_t *bin_slot = nullptr;     // [kNumBins] slot in the LDS image of the power pair of bin (kMinBin + i)
  double *wcos = nullptr;           // [512] cos(theta (i - 256)), theta = 2 pi / 4095: window recurrence seeds
  core::WindowConst wconst;         // fp_core.h window_step
  uint32_t *fold_tab = nullptr;     // [12 * 16] fold thread -> first slot | positions << 16 (fp_core.h PowerLayout)
  core::ClassifierThresholds *thr = nullptr;
  // f32 first pass (stft32_kernel.h): correctly rounded twiddles and window
  core::cf *tw32 = nullptr;         // [4096]
  float *win32 = nullptr;           // [4096] (0.54 - 0.46 cos(theta n)) / 32767 / 2
};

std::mutex g_tab_mu;
std::map<int, FpTables> g_tables;

const double kThresholds[16][3] = {
    {1.98215, 2.35817, 2.63523},          {-1.03809, -0.651211, -0.282167},  {-0.298702, 0.119262, 0.558497},
    {-0.105439, 0.0153946, 0.135898},     {-0.142891, 0.0258736, 0.200632},  {-0.826319, -0.590612, -0.368214},
    {-0.557409, -0.233035, 0.0534525},    {-0.0646826, 0.00620476, 0.0784847}, {-0.192387, -0.029699, 0.215855},
    {-0.0397818, -0.00568076, 0.0292026}, {-0.53823, -0.369934, -0.190235},  {-0.124877, 0.0296483, 0.139239},
    {-0.101475, 0.0225617, 0.231971},     {-0.0799915, -0.00729616, 0.063262}, {-0.272556, 0.019424, 0.302559},
    {-0.164292, -0.0321188, 0.0846339},
};

Status get_tables(FpTables *out) {
  int dev = 0;
  NEEDLE_HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_tab_mu);
  auto it = g_tables.find(dev);
  if (it != g_tables.end()) {
    *out = it->second;
    return Status::Ok();
  }
  std::vector<cd> tw(4096);
  for (int k = 0; k < 4096; k++) {
    long double a = -2.0L * 3.14159265358979323846264338327950288L * k / 4096.0L;
    tw[k] = cd{(double)cosl(a), (double)sinl(a)};
  }
  // chromaprint PrepareHammingWindow(scale = 1/INT16_MAX), times fp_core.h's 2^-1, as recurrence seeds and constants
  const long double theta = 2.0L * 3.14159265358979323846264338327950288L / 4095.0L;
  std::vector<double> wcos(512);
  for (int i = 0; i < 512; i++) wcos[i] = (double)cosl(theta * (long double)(i - 256));
  core::WindowConst wconst;
  wconst.k2 = (double)(2.0L * cosl(256.0L * theta));
  wconst.a = core::kPairInputScale * (0.54 / 32767.0);
  wconst.b = core::kPairInputScale * (0.46 / 32767.0);
  // chromaprint Chroma::PrepareNotes: bin -> pitch class; then where each bin's power pair lives in the LDS image
  // and what each fold lane reads (fp_core.h build_power_layout)
  std::vector<uint8_t> class_of_bin(core::kNumBins);
  for (int i = core::kMinBin; i < core::kMaxBin; i++) {
    double freq = (double)i * kSampleRate / kFrameSize;
    double octave = std::log(freq / (440.0 / 16.0)) / std::log(2.0);
    double note = kBands * (octave - std::floor(octave));
    class_of_bin[i - core::kMinBin] = (uint8_t)(int)(signed char)note;
  }
  auto layout = std::make_unique<core::PowerLayout>();
  if (!core::build_power_layout(class_of_bin.data(), layout.get()))
    return Status::Make(NeedleError_Unknown, "pitch classes do not fit the fold's power layout");
  core::ClassifierThresholds thr;
  for (int i = 0; i < 16; i++)
    for (int j = 0; j < 3; j++) thr.e[i][j] = std::exp(kThresholds[i][j]);

  std::vector<core::cf> tw32(4096);
  std::vector<float> win32(4096);
  for (int k = 0; k < 4096; k++) {
    const long double a = -2.0L * 3.14159265358979323846264338327950288L * k / 4096.0L;
    tw32[k] = core::cf{(float)cosl(a), (float)sinl(a)};
    win32[k] = (float)((long double)core::kPairInputScale * (0.54L - 0.46L * cosl(theta * (long double)k)) / 32767.0L);
  }
  FpTables t;
  t.wconst = wconst;
  auto upload = [](auto **dst, const auto *src, size_t count) -> Status {
    NEEDLE_HIP_TRY(hipMalloc((void **)dst, count * sizeof(**dst)));
    NEEDLE_HIP_TRY(hipMemcpy(*dst, src, count * sizeof(**dst), hipMemcpyHostToDevice));
    return Status::Ok();
  };
  Status s;
  if (!(s = upload(&t.bin_slot, layout->bin_slot, std::size(layout->bin_slot))).ok() ||
      !(s = upload(&t.fold_tab, layout->fold, std::size(layout->fold))).ok() || !(s = upload(&t.tw, tw.data(), tw.size())).ok() ||
      !(s = upload(&t.wcos, wcos.data(), wcos.size())).ok() || !(s = upload(&t.thr, &thr, 1)).ok() ||
      !(s = upload(&t.tw32, tw32.data(), tw32.size())).ok() || !(s = upload(&t.win32, win32.data(), win32.size())).ok())
    return s;
  g_tables[dev] = t;
  *out = t;
  return Status::Ok();
}

// NEEDLE_HIP_STFT_SHARE (hipctx.hip stft_stream): 2 = default, the next job's first pass beside this job's tail; 1 = behind
// this job's recomputation (round-4 measurement); 0 = one stream
int share_mode() {
  static const int mode = [] {
    const char *e = getenv("NEEDLE_HIP_STFT_SHARE");
    return e ? atoi(e) : 2;
  }();
  return mode;
}

// ---- what the three drivers share ------------------------------------------------------------------------------------
// Pairs of frames per chunk of the f64 recomputation (the unit the certification lists): 634 four-pair chunks per
// 28 x 24 min job are two rounds of the 512 workgroup slots; two-pair chunks fit one
#ifndef NEEDLE_CHUNK_PAIRS
#define NEEDLE_CHUNK_PAIRS 2
#endif
constexpr uint32_t kChunkPairs = NEEDLE_CHUNK_PAIRS;

// The certification radius K: 35 x the worst |log v32 - log v64| / S observed (profiles/r03_f32_gate.log).  Read at
// every call: the tests switch it between calls (0 = accept everything).
float cert_k() {
  const char *e = getenv("NEEDLE_HIP_CERT_K");
  return e ? std::max(0.0f, (float)atof(e)) : 64.0f;
}

// The certified f32 first pass is the default; NEEDLE_HIP_STFT=f64 runs the f64 kernel over everything (the arithmetic
// the contract is defined on).
bool f64_mode() {
  const char *e = getenv("NEEDLE_HIP_STFT");
  return e && std::strcmp(e, "f64") == 0;
}

// items per tile of the fused feature + classify kernels: as many (up to 64) as their LDS rows cover
uint32_t tile_items(uint32_t step) { return (uint32_t)std::min<uint64_t>(64, (uint64_t)(kTileRowsMax - 16) / step + 1); }

// `bound` frames per chunk, a workspace bound, unless NEEDLE_HIP_MAX_FRAMES_PER_CHUNK (tests) names another
uint64_t max_frames_per_chunk(uint64_t bound) {
  const char *e = getenv("NEEDLE_HIP_MAX_FRAMES_PER_CHUNK");
  return e ? (uint64_t)std::max(1, atoi(e)) : bound;
}

// The control block of a certified pass whose tail sees `pairs` frame pairs: CertWork, then one bit per chunk.  The
// first pass zeroes all of it in front of the certification.
struct CertLayout {
  uint64_t nchunks;
  size_t ctl_words;
  explicit CertLayout(uint64_t pairs)
      : nchunks((std::max<uint64_t>(pairs, 1) + kChunkPairs - 1) / kChunkPairs),
        ctl_words(sizeof(CertWork) / 4 + (size_t)((nchunks + 31) / 32)) {}
  static CertWork *work(uint32_t *ctl) { return reinterpret_cast<CertWork *>(ctl); }
  static uint32_t *bitmap(uint32_t *ctl) { return ctl + sizeof(CertWork) / 4; }
};

// the buffers of one certified pass: frame energies, control block (CertLayout), the two lists
struct CertBuffers {
  DeviceBuffer<float> energy;
  DeviceBuffer<uint32_t> ctl, chunk_list;
  DeviceBuffer<CertItem> item_list;
  Status reserve(const CertLayout &layout, uint64_t kept, uint64_t energy_frames) {
    Status s;
    if (!(s = energy.reserve(energy_frames * stft::kEnergyParts)).ok() || !(s = ctl.reserve(layout.ctl_words)).ok() ||
        !(s = chunk_list.reserve(layout.nchunks)).ok() || !(s = item_list.reserve(std::max<uint64_t>(kept, 1))).ok())
      return s;
    return Status::Ok();
  }
};

// workspace reused across calls (per device)
struct FpWorkspace {
  DeviceBuffer<double> chroma, feat;
  // Stream tables, one slot per chunk of a call: a job that is run again finds every chunk's table resident and
  // uploads nothing (with a single slot the chunks of a large batch evict each other, and every upload then waits
  // for the staging buffer behind the kernels already queued).
  struct Descriptors {
    DeviceBuffer<FpStream> streams;
    PinnedStage stage;
    DescriptorUpload<FpStream> upload;
  };
  static constexpr size_t kDescriptorSlots = 64;
  std::vector<std::unique_ptr<Descriptors>> descriptors;
  Descriptors &slot(size_t chunk) {
    const size_t k = chunk % kDescriptorSlots;
    if (descriptors.size() <= k) descriptors.resize(k + 1);
    if (!descriptors[k]) descriptors[k] = std::make_unique<Descriptors>();
    return *descriptors[k];
  }
  bool lds_attr_set = false;  // the STFT kernel's 68 KiB of dynamic LDS needs an explicit opt-in
  Descriptors feed_first, feed_second;  // the two tables of a feed (gpu_fingerprint_feed_device)
  CertBuffers cert;  // certified first pass (a feed brings its own energy rows)
  // the same set twice more for calls that are pipelined two deep (gpu_fingerprint_device's `pipe`): the STFT of call
  // k + 1 writes its chroma while the certification / recomputation / fix-up of call k still read theirs
  struct Pipe {
    DeviceBuffer<double> chroma;
    CertBuffers cert;
    hipEvent_t stft_begin = nullptr, stft_done = nullptr;  // bound to the first pass's own dispatch (no marker packets)
    hipEvent_t recomputed = nullptr;  // recorded on the library stream behind the f64 recomputation of the listed chunks
    hipEvent_t consumed = nullptr;    // recorded on the library stream behind the last reader of this set
    hipEvent_t descriptors = nullptr; // recorded on the library stream behind a descriptor upload the STFT must see
    bool consumed_valid = false, stft_recorded = false;
  } pipes[2];
  CertStats *stats = nullptr;                     // device, cumulative
  uint64_t items_total = 0, chunks_total = 0;     // host: what the device counts are fractions of
};
FpWorkspace *workspace() {  // (never destroyed: HIP may already be gone when static destructors run)
  static std::mutex mu;
  static std::map<int, FpWorkspace *> all;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  FpWorkspace *&w = all[dev];
  if (!w) w = new FpWorkspace();
  return w;
}

// ---- stream tables -----------------------------------------------------------------------------------------------------
// FpStream (stft_kernel.h) as the kernels read it.  Every *_base is the prefix sum of its quantity over the table's
// earlier streams, and is what find_stream searches: frame_base of frames = the stream's first chroma / energy row,
// pair_base of ceil(frames / 2) (stft_chroma*, and the chunks of the recomputation), fir_base of fir_rows (fir_norm,
// classify), kept_base of kept (classify), tile_base of ceil(kept / items_per_tile) (features_classify*, audit_items).
// In a feed's tables frame_base is the lane's place in the feeder's row buffers instead, and fir_base doubles as the
// PHASED item phase: the rows from the stream's first frame to its first kept item (plan_feed).

// One chunk of a call: the streams [begin, end) of `spans`, as many as stay within max_frames frames (at least one).
struct ChunkPlan {
  size_t end = 0;
  std::vector<FpStream> streams;
  uint64_t frames = 0, rows = 0, kept = 0, pairs = 0, tiles = 0;
};
Status plan_chunk(const std::vector<StreamSpan> &spans, size_t begin, int channels, uint32_t step, uint32_t items_per_tile,
                  uint64_t max_frames, ChunkPlan *plan) {
  *plan = ChunkPlan{};
  size_t end = begin;
  for (; end < spans.size(); end++) {
    const size_t samples = spans[end].num_values / (size_t)channels;
    const uint64_t f = num_frames(samples);
    if (!plan->streams.empty() && plan->frames + f > max_frames) break;
    if (f > 0xFFFFFFF0ull) return Status::Make(NeedleError_InvalidArgument, "fingerprint: stream too long");
    FpStream m;
    m.pcm_off = spans[end].pcm_off;
    m.item_off = spans[end].item_off;
    m.frames = (uint32_t)f;
    m.frame_base = (uint32_t)plan->frames;
    m.fir_rows = f >= (uint64_t)kFirTaps ? (uint32_t)(f - (kFirTaps - 1)) : 0;
    m.fir_base = (uint32_t)plan->rows;
    m.kept = (uint32_t)num_kept(samples, step);
    m.kept_base = (uint32_t)plan->kept;
    m.pair_base = (uint32_t)plan->pairs;
    m.tile_base = (uint32_t)plan->tiles;
    plan->tiles += (m.kept + items_per_tile - 1) / items_per_tile;
    plan->pairs += (m.frames + 1) / 2;
    plan->frames += m.frames;
    plan->rows += m.fir_rows;
    plan->kept += m.kept;
    plan->streams.push_back(m);
  }
  plan->end = end;
  return Status::Ok();
}

// The two tables of a feed.  `first`: the NEW frame pairs of every lane that has any, for the first pass alone (frames,
// rows and pairs; nothing is classified from it).  `second`: carried + new frames of every lane with new items, for
// certification, recomputation and fix-up, the lane's first new item `first_item` rows in (PHASED).
struct FeedPlan {
  std::vector<FpStream> first, second;
  std::vector<uint32_t> second_lane;  // the feeder's lane of every stream of `second` (an audited feed counts by it)
  uint64_t pairs1 = 0, pairs2 = 0, kept = 0, tiles = 0;
  uint64_t chunks1 = 0;  // chunks of the new pairs: what a feed adds to the count the recomputed chunks are a fraction of
};
Status plan_feed(const std::vector<FeedLane> &lanes, int channels, uint32_t step, uint32_t items_per_tile, FeedPlan *plan) {
  *plan = FeedPlan{};
  for (const FeedLane &l : lanes) {
    if (l.frames < l.carried || (l.carried & 1u)) return Status::Make(NeedleError_InvalidArgument, "fingerprint: a feed's carried rows must be an even prefix");
    const uint32_t fresh = l.frames - l.carried;
    if (fresh) {
      FpStream m{};
      m.pcm_off = l.pcm_off + (uint64_t)l.carried * kHop * (uint64_t)channels;
      m.frames = fresh;
      m.frame_base = l.row_base + l.carried;
      m.pair_base = (uint32_t)plan->pairs1;
      plan->pairs1 += (fresh + 1) / 2;
      plan->chunks1 += ((fresh + 1) / 2 + kChunkPairs - 1) / kChunkPairs;
      plan->first.push_back(m);
    }
    if (l.kept) {
      if ((uint64_t)l.first_item + (uint64_t)(l.kept - 1) * step + kItemLatency + 1 > l.frames)
        return Status::Make(NeedleError_InvalidArgument, "fingerprint: a feed's items reach past its frames");
      FpStream m{};
      m.pcm_off = l.pcm_off;
      m.item_off = l.item_off;
      m.frames = l.frames;
      m.frame_base = l.row_base;
      m.fir_base = l.first_item;  // PHASED: not a prefix of FIR rows here
      m.kept = l.kept;
      m.kept_base = (uint32_t)plan->kept;
      m.pair_base = (uint32_t)plan->pairs2;
      m.tile_base = (uint32_t)plan->tiles;
      plan->tiles += (l.kept + items_per_tile - 1) / items_per_tile;
      plan->pairs2 += (l.frames + 1) / 2;
      plan->kept += l.kept;
      plan->second.push_back(m);
      plan->second_lane.push_back(l.lane);
    }
  }
  return Status::Ok();
}

// ---- taps (test hook) --------------------------------------------------------------------------------------------------
// needle_hip_fingerprint_stages_debug: a certified call that is given taps fills its chroma and energy rows with a NaN
// bit pattern in front of the first pass and copies, device to device and in stream order BETWEEN the launches it makes
// anyway, what each of its four kernels wrote.  No launch, grid or argument differs from the call without taps, except
// that `beside` picks the listed kernel's other form and that a batch without a single kept item still runs its first pass.
struct FpTaps {
  bool beside = false;  // in: the recomputation in the form that fits beside a first pass (stft_variant(channels, true, true))
  DeviceBuffer<double> first_chroma, final_chroma;  // [frames][12] behind the first pass / behind the recomputation
  DeviceBuffer<float> energy;                       // [frames][kEnergyParts] behind the first pass
  DeviceBuffer<uint32_t> first_items;               // [kept] behind the certification, in front of the fix-up
  DeviceBuffer<uint32_t> ctl, chunk_list;           // the control block (CertLayout) and the chunk list behind the certification
  DeviceBuffer<CertItem> item_list;
  std::vector<FpStream> streams;                    // the call's one chunk, as plan_chunk numbered it
  uint64_t frames = 0, pairs = 0, kept = 0, nchunks = 0;
  size_t ctl_words = 0;
  uint32_t items_per_tile = 0, pairs_per_block = 0;
  Stft32Schedule schedule;
  bool ran = false;  // false: a batch without a frame, nothing was launched
};
template <typename T>
Status tap_copy(T *dst, const T *src, uint64_t count, hipStream_t stream) {
  if (count) NEEDLE_HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToDevice, stream));
  return Status::Ok();
}

// ---- launches ----------------------------------------------------------------------------------------------------------
// what every launch of a call is given
struct Job {
  const FpTables &tab;
  const int16_t *d_pcm;
  int channels;
  uint32_t step, items_per_tile;
  uint32_t *d_items;
  hipStream_t stream;  // the library stream
};
struct Table {  // a stream table on the device
  const FpStream *streams;
  int n;
  uint64_t pairs;
};

// Every instantiated variant of stft_chroma_kernel: over the whole table, or LISTED (the recomputation), that one also
// in the 168-VGPR form that fits BESIDE the next job's first pass (stft_kernel.h WAVES).
using StftKernel = decltype(&stft_chroma_kernel<1, 0, false>);
StftKernel stft_variant(int channels, bool listed, bool beside) {
  if (!listed) return channels == 1 ? stft_chroma_kernel<1, 0, false> : stft_chroma_kernel<2, 0, false>;
  if (beside) return channels == 1 ? stft_chroma_kernel<1, 0, true, 3> : stft_chroma_kernel<2, 0, true, 3>;
  return channels == 1 ? stft_chroma_kernel<1, 0, true> : stft_chroma_kernel<2, 0, true>;
}

// the f64 STFT kernel's 68 KiB of dynamic LDS needs an explicit opt-in, once per device
Status stft_lds_opt_in() {
  FpWorkspace *ws = workspace();
  if (ws->lds_attr_set) return Status::Ok();
  for (int channels = 1; channels <= 2; channels++)
    for (int form = 0; form < 3; form++)
      NEEDLE_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(stft_variant(channels, form > 0, form > 1)),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)(core::kLds2Slots * sizeof(cd))));
  ws->lds_attr_set = true;
  return Status::Ok();
}

void launch_stft_chroma(const Job &j, StftKernel kernel, uint32_t grid, const Table &t, double *chroma, uint32_t pairs_per_block,
                        stft::ChunkList list) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), core::kLds2Slots * sizeof(cd), j.stream, j.d_pcm, t.streams, t.n, j.tab.tw,
                     j.tab.wcos, j.tab.wconst, j.tab.bin_slot, j.tab.fold_tab, chroma, (uint32_t)t.pairs, pairs_per_block, list);
}

// The f32 first pass over the pairs of `table`: their chroma and energy rows, and `ctl_words` words of `ctl` zeroed.
struct FirstPass {
  Table table;
  Stft32Schedule schedule;
  double *chroma;
  float *energy;
  uint32_t *ctl;
  uint32_t ctl_words;
  hipStream_t on;  // the library stream, or the pipe's own
  // A pipelined call's first pass carries its events in its own dispatch packet (hipExtLaunchKernelGGL): the
  // completion signal of the kernel is `stft_done`, what the library stream waits for, and nothing but the kernel
  // sits between two first passes on their stream (event records around it were 13 us per job).
  FpWorkspace::Pipe *pipe;
  bool timed;      // no pipe: KernelTimer's event records around the launch
};
Status enqueue_first_pass(const Job &j, const FirstPass &f) {
  FpWorkspace::Pipe *pp = f.pipe;
  const bool bound_timing = pp != nullptr && kernel_timing_on("stft_chroma32");
  std::unique_ptr<KernelTimer> timer;
  if (!pp && f.timed) timer.reset(new KernelTimer("stft_chroma32", f.on));
  Status s = launch_stft_chroma32(j.channels, f.schedule, f.on, j.d_pcm, f.table.streams, f.table.n, j.tab.tw32, j.tab.win32,
                                  j.tab.bin_slot, j.tab.fold_tab, f.chroma, f.energy, (uint32_t)f.table.pairs, f.ctl, f.ctl_words,
                                  bound_timing ? pp->stft_begin : nullptr, pp ? pp->stft_done : nullptr);
  if (!s.ok()) return s;
  if (bound_timing) bind_kernel_events("stft_chroma32", pp->stft_begin, pp->stft_done);
  return Status::Ok();
}

// The certified chain: first pass, certification of the tail table's items, f64 recomputation of the listed chunks,
// fix-up of the listed items.
struct CertChain {
  FirstPass first;       // no pairs (a feed that only finishes its lanes): the control block is cleared by a memset; its
                         // ctl / ctl_words are the chain's control block (CertLayout)
  Table tail;            // what certification, recomputation and fix-up see; one-shot: the first pass's table
  uint64_t tiles, kept;  // of the tail; no tiles: the first pass alone
  bool phased;           // the tail's items start fir_base rows into their streams (a feed)
  double *recomputed;    // where the recomputation writes and the fix-up reads: the first pass's chroma itself, or rows of
                         // their own with the same numbering (a feed keeps the first pass's rows for the next feed)
  CertBuffers *bufs;
  uint32_t fallback_grid;
  bool beside;           // the recomputation in the form that fits beside the next job's first pass
  uint32_t *zero_word;   // cleared by the fix-up, or nullptr
  uint64_t count_chunks; // added to the chunks the recomputed ones are a fraction of
  FpTaps *taps = nullptr;  // test hook: copies between the launches (FpTaps); the product passes none
};
Status enqueue_certified(const Job &j, FpWorkspace *ws, const CertChain &c, bool *zeroed) {
  hipStream_t stream = j.stream;
  FpWorkspace::Pipe *pp = c.first.pipe;
  if (!ws->stats) {
    NEEDLE_HIP_TRY(hipMalloc((void **)&ws->stats, sizeof(CertStats)));
    NEEDLE_HIP_TRY(hipMemsetAsync(ws->stats, 0, sizeof(CertStats), stream));
  }
  CertWork *work = CertLayout::work(c.first.ctl);
  FpTaps *tap = c.taps;
  Status ts;
  if (tap) {  // a row no kernel writes stays a NaN
    NEEDLE_HIP_TRY(hipMemsetAsync(c.first.chroma, 0xFF, tap->frames * kBands * sizeof(double), c.first.on));
    NEEDLE_HIP_TRY(hipMemsetAsync(c.first.energy, 0xFF, tap->frames * stft::kEnergyParts * sizeof(float), c.first.on));
  }
  if (c.first.table.pairs) {
    Status s = enqueue_first_pass(j, c.first);
    if (!s.ok()) return s;
    if (tap && (!(ts = tap_copy(tap->first_chroma.ptr, c.first.chroma, tap->frames * kBands, c.first.on)).ok() ||
                !(ts = tap_copy(tap->energy.ptr, c.first.energy, tap->frames * stft::kEnergyParts, c.first.on)).ok()))
      return ts;
  } else {
    NEEDLE_HIP_TRY(hipMemsetAsync(c.first.ctl, 0, c.first.ctl_words * sizeof(uint32_t), stream));
  }
  if (pp) {  // everything behind the first pass stays on the library stream, behind the STFT's event
    pp->stft_recorded = true;
    NEEDLE_HIP_TRY(hipStreamWaitEvent(stream, pp->stft_done, 0));
  }
  ws->chunks_total += c.count_chunks;
  if (c.tiles) {
    {
      KernelTimer timer("features_cert");
      // SPLIT exactly at step 2 (a feed too: an even step's items start at even rows of the even-aligned carried region)
      const bool split = j.step == 2;
      hipLaunchKernelGGL(c.phased ? (split ? features_classify_cert_kernel<true, true> : features_classify_cert_kernel<false, true>)
                                  : (split ? features_classify_cert_kernel<true> : features_classify_cert_kernel<false>),
                         dim3((uint32_t)((c.tiles + kCertWaves - 1) / kCertWaves)), dim3(64 * kCertWaves), 0, stream, c.first.chroma,
                         c.first.energy, c.tail.streams, c.tail.n, j.tab.thr, j.step, j.items_per_tile, j.d_items, (uint32_t)c.tiles,
                         cert_k(), kChunkPairs, work, CertLayout::bitmap(c.first.ctl), c.bufs->chunk_list.ptr, c.bufs->item_list.ptr);
    }
    if (tap && (!(ts = tap_copy(tap->first_items.ptr, j.d_items, tap->kept, stream)).ok() ||
                !(ts = tap_copy(tap->chunk_list.ptr, c.bufs->chunk_list.ptr, tap->nchunks, stream)).ok() ||
                !(ts = tap_copy(tap->item_list.ptr, c.bufs->item_list.ptr, tap->kept, stream)).ok()))
      return ts;
    {
      KernelTimer timer("stft_fallback");
      launch_stft_chroma(j, stft_variant(j.channels, true, c.beside), c.fallback_grid, c.tail, c.recomputed, kChunkPairs,
                         stft::ChunkList{c.bufs->chunk_list.ptr, &work->chunk_count});
    }
    if (tap && !(ts = tap_copy(tap->final_chroma.ptr, c.recomputed, tap->frames * kBands, stream)).ok()) return ts;
    if (pp) NEEDLE_HIP_TRY(hipEventRecord(pp->recomputed, stream));
#ifndef NEEDLE_LAB_NO_FIXUP   // (timing laboratory, WRONG results: the job without the fix-up's dispatch -- the most that folding it into the recomputation kernel could save)
    {
      KernelTimer timer("fixup_items");
      hipLaunchKernelGGL(fixup_items_kernel, dim3(64), dim3(256), 0, stream, c.recomputed, j.tab.thr, work, c.bufs->item_list.ptr,
                         j.d_items, ws->stats, c.zero_word);
      *zeroed = c.zero_word != nullptr;
    }
#endif
    if (pp) {
      NEEDLE_HIP_TRY(hipEventRecord(pp->consumed, stream));
      pp->consumed_valid = true;
    }
    ws->items_total += c.kept;
  } else if (tap && !(ts = tap_copy(tap->final_chroma.ptr, c.recomputed, tap->frames * kBands, stream)).ok()) {
    return ts;  // (no item: the first pass's rows are the call's last)
  }
  if (tap && !(ts = tap_copy(tap->ctl.ptr, c.first.ctl, tap->ctl_words, stream)).ok()) return ts;  // nothing behind the certification writes it
  NEEDLE_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

// The f64 chain: the transform over the pairs of `first`, then feature rows + classifiers over the tiles of `tail`.
struct F64Chain {
  Table first;
  uint32_t pairs_per_block;
  double *chroma;
  Table tail;      // one-shot: `first` again
  uint64_t tiles;  // 0: the caller looks at the chroma by other means (the audit; a call that wants the features)
  bool phased;     // as CertChain
  bool timed;
};
Status enqueue_f64(const Job &j, const F64Chain &c) {
  if (c.first.pairs) {
    std::unique_ptr<KernelTimer> timer;
    if (c.timed) timer.reset(new KernelTimer("stft_chroma"));
    const uint32_t ppb = c.pairs_per_block;
    const uint32_t grid = (uint32_t)(((c.first.pairs + ppb - 1) / ppb + 7) / 8 * 8);  // multiple of 8: see the XCD mapping
    launch_stft_chroma(j, stft_variant(j.channels, false, false), grid, c.first, c.chroma, ppb, stft::ChunkList{nullptr, nullptr});
  }
  if (c.tiles) {
    KernelTimer timer("features_classify");
    hipLaunchKernelGGL(c.phased ? features_classify_kernel<true> : features_classify_kernel<false>, dim3((uint32_t)((c.tiles + 3) / 4)),
                       dim3(256), 0, j.stream, c.chroma, c.tail.streams, c.tail.n, j.tab.thr, j.step, j.items_per_tile, j.d_items,
                       (uint32_t)c.tiles);
  }
  NEEDLE_HIP_TRY(hipGetLastError());
  return Status::Ok();
}

// ---- the one-shot driver's own -----------------------------------------------------------------------------------------
// Pairs per workgroup.  The device holds `slots` workgroups at a time.  A launch of more than
// about two rounds of workgroups balances itself (workgroups retire at different times and the dispatcher
// backfills: measured, a "whole rounds" choice of the size changed 7- and 14-episode launches by < 2 %), so
// long launches keep kPairsPerBlock.  A SHORT launch -- one rank's share of a sharded job, a single file --
// is cut so that every slot gets one workgroup: 4 episodes x 24 min = 11 626 pairs run as 506 workgroups of
// 23 pairs (0.153 ms) instead of 727 of 16 (0.162 ms); one episode as 485 workgroups of 6 instead of 182 of 16.
uint32_t launch_pairs_per_block(uint64_t pairs, uint64_t slots, uint32_t long_launch = kPairsPerBlock) {
  uint32_t ppb = long_launch;
  if (pairs < (long_launch > (uint32_t)kPairsPerBlock ? 40 : 2 * kPairsPerBlock) * slots)
    ppb = (uint32_t)std::min<uint64_t>(40, std::max<uint64_t>(4, (pairs + slots - 1) / slots));
  if (const char *e = getenv("NEEDLE_STFT_PAIRS")) ppb = (uint32_t)std::max(1, atoi(e));
  return ppb;
}

// What a pipelined first pass on `stft` waits for before it may start (events of the pipes, created on first use).
Status order_pipelined_first_pass(FpWorkspace *ws, int pipe, hipStream_t stft, hipStream_t stream, bool uploaded) {
  FpWorkspace::Pipe *pp = &ws->pipes[pipe];
  for (hipEvent_t *e : {&pp->consumed, &pp->descriptors, &pp->recomputed})
    if (!*e) NEEDLE_HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
  for (hipEvent_t *e : {&pp->stft_begin, &pp->stft_done})  // these two also time the kernel (KernelTimer's role)
    if (!*e) NEEDLE_HIP_TRY(hipEventCreate(e));
  // the STFT may start once the previous user of this workspace has read it to the end, and -- only if the
  // descriptor table was uploaded just now -- once that copy has executed (an unconditional wait on the library
  // stream would put the STFT behind the whole previous job, which is the one thing this is here to avoid)
  // (an event that has completed by now needs no packet in the STFT's queue: nothing but the previous first pass
  // should sit in front of this one)
  if (pp->consumed_valid) {
    if (hipEventQuery(pp->consumed) != hipSuccess) {
      (void)hipGetLastError();
      NEEDLE_HIP_TRY(hipStreamWaitEvent(stft, pp->consumed, 0));
    }
  }
  // ... and once the OTHER pipe's first pass is through: two STFTs side by side only slow each other down and
  // leave both tails to run alone afterwards (seen in a kernel trace: pairs of 0.67 / 0.76 ms STFTs, then 0.2 ms
  // of tail kernels on an idle chip); what is wanted beside an STFT is the previous call's TAIL
  // Shared-CU overlap (NEEDLE_HIP_STFT_SHARE, hipctx.hip): behind the other pipe's f64 RECOMPUTATION instead.  That
  // kernel's workgroup (68 KB of LDS, ~250 VGPRs) does not fit the hole a retiring first-pass workgroup leaves
  // (35 KB, 163 VGPRs): started beside a first pass it waits for all of it (kernel trace, profiles/NOTES.md round 4);
  // the kernels behind it (fix-up, scan, simhash) and the certification kernel do fit and run beside it.
  const FpWorkspace::Pipe &other = ws->pipes[pipe ^ 1];
  const bool share = share_mode() == 1;  // (default, 2: behind the first pass only)
  if (share && other.recomputed && other.stft_recorded)
    NEEDLE_HIP_TRY(hipStreamWaitEvent(stft, other.recomputed, 0));
  else if (share_mode() != 2 && other.stft_done && other.stft_recorded)  // (2: both on one stream, in order anyway)
    NEEDLE_HIP_TRY(hipStreamWaitEvent(stft, other.stft_done, 0));
  if (uploaded) {
    NEEDLE_HIP_TRY(hipEventRecord(pp->descriptors, stream));
    NEEDLE_HIP_TRY(hipStreamWaitEvent(stft, pp->descriptors, 0));
  }
  return Status::Ok();
}

// what every driver starts with, under gpu_mutex()
Status begin_call(int channels, uint32_t step, FpTables *tab) {
  if (channels != 1 && channels != 2) return Status::Make(NeedleError_InvalidArgument, "fingerprint: channels must be 1 or 2");
  if (step == 0) return Status::Make(NeedleError_InvalidArgument, "fingerprint: step must be >= 1");
  Status s = ensure_device();
  if (!s.ok() || !(s = get_tables(tab)).ok() || !(s = stft_lds_opt_in()).ok()) return s;
  return Status::Ok();
}

// gpu_fingerprint_device, and the same call with taps (gpu_fingerprint_stages_debug)
Status fingerprint_device(const int16_t *d_pcm, const std::vector<StreamSpan> &spans, int channels, uint32_t step, uint32_t *d_items,
                          bool sync, double *d_chroma_dbg, double *d_feat_dbg, size_t descriptor_slot, int pipe, uint32_t *zero_word,
                          bool *zeroed_out, FpTaps *taps) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  bool zeroed = false;  // *zero_word was cleared by the LAST kernel enqueued here (only then is it still zero for the caller)
  if (zeroed_out) *zeroed_out = false;
  FpTables tab;
  Status s = begin_call(channels, step, &tab);
  if (!s.ok()) return s;
  hipStream_t stream = library_stream();
  FpWorkspace *ws = workspace();
  const uint64_t cus = (uint64_t)device_cu_count();

  // Streams are processed in chunks so the f64 chroma/feature workspaces stay bounded (96 B/frame each):
  // 8 M frames = 0.8 GB of chroma + as much of features
  const uint64_t max_frames = max_frames_per_chunk(8u << 20);
  uint32_t items_per_tile = tile_items(step);
  if (const char *e = getenv("NEEDLE_HIP_ITEMS_PER_TILE")) items_per_tile = std::min(items_per_tile, (uint32_t)std::max(1, atoi(e)));  // tuning
  const Job job{tab, d_pcm, channels, step, items_per_tile, d_items, stream};
  // The f64 kernel over everything also when a caller asks for the intermediate stages
  const bool separate = d_feat_dbg != nullptr || getenv("NEEDLE_HIP_SEPARATE_CLASSIFY") != nullptr;
  const bool certifiable = !f64_mode() && d_chroma_dbg == nullptr && !separate;
  if (taps && !certifiable) return Status::Make(NeedleError_InvalidArgument, "fingerprint: the stages of the certified chain were asked for, and this call does not run it");
  size_t begin = 0, chunk = descriptor_slot;
  while (begin < spans.size()) {
    ChunkPlan plan;
    if (!(s = plan_chunk(spans, begin, channels, step, items_per_tile, max_frames, &plan)).ok()) return s;
    const bool whole = begin == 0 && plan.end == spans.size();
    if (taps && !whole) return Status::Make(NeedleError_InvalidArgument, "fingerprint: the stages of a batch of more than one chunk were asked for");
    begin = plan.end;
    const uint64_t frames = plan.frames, pairs = plan.pairs, tiles = plan.tiles;
    if (frames == 0) continue;
    const bool certified = certifiable && (tiles > 0 || taps);
    // Pipelined call (pipe 0 / 1) small enough to be ONE chunk, with a CU-masked stream available: its f32 STFT goes
    // to that stream and its own workspace; otherwise everything stays on the library stream.
    hipStream_t stft = certified && (pipe == 0 || pipe == 1) && whole && frames <= (1u << 21) ? stft_stream() : nullptr;
    FpWorkspace::Pipe *pp = stft ? &ws->pipes[pipe] : nullptr;
    if (pp) {
      // ... and only while the OTHER pipe still has work queued: a call that is alone on the device keeps all CUs
      // (same workspace and events, the first pass simply stays on the library stream)
      const FpWorkspace::Pipe &other = ws->pipes[pipe ^ 1];
      const bool busy = other.consumed_valid && hipEventQuery(other.consumed) == hipErrorNotReady;
      (void)hipGetLastError();
      if (!busy) stft = stream;
      if (getenv("NEEDLE_HIP_TRACE"))
        std::fprintf(stderr, "[needle_hip] pipelined first pass: pipe %d, %s\n", pipe,
                     stft != stream ? "beside the other pipe" : "alone on the library stream");
    }
    DeviceBuffer<double> &chroma_buf = pp ? pp->chroma : ws->chroma;
    if (!(s = chroma_buf.reserve(frames * kBands)).ok()) return s;
    if (!pp && !(s = ws->feat.reserve(std::max<uint64_t>(plan.rows, 1) * kBands)).ok()) return s;
    // (a pipelined call gets descriptor slots of its own: the other pipe's table must stay resident)
    FpWorkspace::Descriptors &desc = ws->slot(pp ? FpWorkspace::kDescriptorSlots - 2 + (size_t)pipe : chunk++);
    bool uploaded = false;
    if (!(s = desc.upload.put(&desc.streams, &desc.stage, plan.streams, stream, &uploaded)).ok()) return s;
    const Table table{desc.streams.ptr, (int)plan.streams.size(), pairs};
    if (certified) {
      const CertLayout layout(pairs);
      CertBuffers &bufs = pp ? pp->cert : ws->cert;
      if (!(s = bufs.reserve(layout, plan.kept, frames)).ok()) return s;
      if (pp && !(s = order_pipelined_first_pass(ws, pipe, stft, stream, uploaded)).ok()) return s;
      const uint64_t slots = (uint64_t)kStft32WavesPerSimd * cus;
      // Long launches: 24 pairs per workgroup and, over the last half round of every XCD's part, 12, 6 and 3
      // (stft32_schedule.h): fewer workgroup prologues in the bulk, a short ramp at the end; 0.463 -> 0.453 ms alone at
      // 28 x 24 min against 16 throughout (profiles/NOTES.md).  NEEDLE_STFT_GUIDED: tenths of a round, 0 = off.
      static const int guided = getenv("NEEDLE_STFT_GUIDED") ? atoi(getenv("NEEDLE_STFT_GUIDED")) : 5;
      const uint32_t ppb = launch_pairs_per_block(pairs, slots, guided > 0 ? 24u : (uint32_t)kPairsPerBlock);
      // A pipelined call runs BESIDE the next call's first pass (shared-CU overlap): then the 168-VGPR form, whose
      // workgroup fits the hole one retiring first-pass workgroup leaves (the 229-VGPR form needs two and waited a whole
      // first pass for them), on a quarter of the workgroups (each holds its slot for its whole, latency-bound life).
      const bool beside = (pp != nullptr && share_mode() == 2 && stft_stream() != nullptr) || (taps && taps->beside);
      uint32_t grid = (uint32_t)std::min<uint64_t>((beside ? 1ull : 4ull) * cus / 2, layout.nchunks);
      if (const char *e = getenv("NEEDLE_HIP_FALLBACK_GRID")) grid = (uint32_t)std::min<uint64_t>((uint64_t)std::max(1, atoi(e)), layout.nchunks);  // tuning
      const FirstPass first{table, stft32_schedule(pairs, ppb, (slots + 7) / 8, guided > 0, (uint32_t)std::max(guided, 1)),
                            chroma_buf.ptr, bufs.energy.ptr, bufs.ctl.ptr, (uint32_t)layout.ctl_words, pp ? stft : stream, pp, true};
      if (taps) {
        taps->streams = plan.streams;
        taps->frames = frames, taps->pairs = pairs, taps->kept = plan.kept, taps->nchunks = layout.nchunks;
        taps->ctl_words = layout.ctl_words;
        taps->items_per_tile = items_per_tile, taps->pairs_per_block = ppb;
        taps->schedule = first.schedule;
        taps->ran = true;
        if (!(s = taps->first_chroma.reserve(frames * kBands)).ok() || !(s = taps->final_chroma.reserve(frames * kBands)).ok() ||
            !(s = taps->energy.reserve(frames * stft::kEnergyParts)).ok() || !(s = taps->first_items.reserve(plan.kept)).ok() ||
            !(s = taps->item_list.reserve(plan.kept)).ok() || !(s = taps->ctl.reserve(layout.ctl_words)).ok() ||
            !(s = taps->chunk_list.reserve(layout.nchunks)).ok())
          return s;
      }
      if (!(s = enqueue_certified(job, ws, CertChain{first, table, tiles, plan.kept, false, chroma_buf.ptr, &bufs, grid, beside,
                                                     zero_word, layout.nchunks, taps}, &zeroed)).ok())
        return s;
      continue;
    }
    zeroed = false;
    if (!(s = enqueue_f64(job, F64Chain{table, launch_pairs_per_block(pairs, 2 * cus), ws->chroma.ptr, table, separate ? 0 : tiles, false, true})).ok())
      return s;
    if (separate) {  // a caller wants the features themselves (tests): kernels 2 and 3 one after the other
      if (plan.rows > 0) {
        KernelTimer timer("fir_norm");
        hipLaunchKernelGGL(fir_norm_kernel, dim3((uint32_t)((plan.rows + 255) / 256)), dim3(256), 0, stream,
                           ws->chroma.ptr, table.streams, table.n, ws->feat.ptr, (uint32_t)plan.rows);
      }
      if (plan.kept > 0) {
        KernelTimer timer("classify");
        hipLaunchKernelGGL(classify_kernel, dim3((uint32_t)((plan.kept + 255) / 256)), dim3(256), 0, stream,
                           ws->feat.ptr, table.streams, table.n, tab.thr, step, d_items, (uint32_t)plan.kept);
      }
      NEEDLE_HIP_TRY(hipGetLastError());
    }
    if (d_chroma_dbg)
      NEEDLE_HIP_TRY(hipMemcpyAsync(d_chroma_dbg, ws->chroma.ptr, frames * kBands * sizeof(double),
                                    hipMemcpyDeviceToDevice, stream));
    if (d_feat_dbg && plan.rows)
      NEEDLE_HIP_TRY(hipMemcpyAsync(d_feat_dbg, ws->feat.ptr, plan.rows * kBands * sizeof(double),
                                    hipMemcpyDeviceToDevice, stream));
    // the next chunk reuses the chroma / feature workspaces: safe without a host wait, the stream runs in order
    // (and every chunk has its own descriptor slot)
  }
  if (zeroed_out) *zeroed_out = zeroed;
  if (sync) NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  return Status::Ok();
}

}  // namespace

Status gpu_fingerprint_device(const int16_t *d_pcm, const std::vector<StreamSpan> &spans, int channels,
                              uint32_t step, uint32_t *d_items, bool sync, double *d_chroma_dbg,
                              double *d_feat_dbg, size_t descriptor_slot, int pipe, uint32_t *zero_word, bool *zeroed_out) {
  return fingerprint_device(d_pcm, spans, channels, step, d_items, sync, d_chroma_dbg, d_feat_dbg, descriptor_slot, pipe, zero_word,
                            zeroed_out, nullptr);
}

// Test hook (include/needle_hip.h needle_hip_fingerprint_stages_debug): host PCM into an arena of its own, the product's
// certified chain over it as ONE chunk with taps, and what the taps hold copied to the host.
Status gpu_fingerprint_stages_debug(const std::vector<const int16_t *> &pcm, const std::vector<size_t> &num_values, int channels,
                                    uint32_t step, uint32_t flags, NeedleHipStages *out) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  if (flags & ~1u) return Status::Make(NeedleError_InvalidArgument, "fingerprint: unknown stage flags");
  if (channels != 1 && channels != 2) return Status::Make(NeedleError_InvalidArgument, "fingerprint: channels must be 1 or 2");
  if (step == 0) return Status::Make(NeedleError_InvalidArgument, "fingerprint: step must be >= 1");
  Status s = ensure_device();
  if (!s.ok()) return s;
  const size_t n = pcm.size();
  std::vector<StreamSpan> spans(n);
  uint64_t values = 0, kept = 0;
  for (size_t i = 0; i < n; i++) {  // streams 16-byte aligned in the arena and items back to back, as fingerprint_in_batches lays them
    spans[i] = StreamSpan{values, num_values[i], kept};
    values += (num_values[i] + 7) & ~(uint64_t)7;
    kept += num_kept(num_values[i] / (size_t)channels, step);
  }
  DeviceBuffer<int16_t> d_pcm;
  DeviceBuffer<uint32_t> d_items;
  if (!(s = d_pcm.reserve(std::max<uint64_t>(values, 1))).ok() || !(s = d_items.reserve(std::max<uint64_t>(kept, 1))).ok()) return s;
  for (size_t i = 0; i < n; i++)
    if (num_values[i]) NEEDLE_HIP_TRY(hipMemcpy(d_pcm.ptr + spans[i].pcm_off, pcm[i], num_values[i] * sizeof(int16_t), hipMemcpyHostToDevice));
  FpTaps taps;
  taps.beside = (flags & 1u) != 0;
  if (!(s = fingerprint_device(d_pcm.ptr, spans, channels, step, d_items.ptr, true, nullptr, nullptr, 0, -1, nullptr, nullptr, &taps)).ok())
    return s;
  out->frames = out->pairs = out->kept = out->chunks = out->items_listed = out->chunks_listed = 0;
  out->chunk_pairs = kChunkPairs;
  out->items_per_tile = taps.items_per_tile;
  out->pairs_per_block = taps.pairs_per_block;
  out->compute_units = (uint32_t)device_cu_count();
  out->pairs_per_xcd = out->blocks_per_xcd = 0;
  for (int k = 0; k < 4; k++) out->block_size[k] = 0, out->block_count[k] = 0;
  if (out->streams)
    for (size_t i = 0; i < n; i++) out->streams[i] = NeedleHipStageStream{0, 0, 0, 0, 0, 0};
  if (!taps.ran) return Status::Ok();  // not one frame in the batch
  out->frames = taps.frames, out->pairs = taps.pairs, out->kept = taps.kept, out->chunks = taps.nchunks;
  out->pairs_per_xcd = taps.schedule.pairs_per_xcd, out->blocks_per_xcd = taps.schedule.blocks_per_xcd;
  for (int k = 0; k < 4; k++) out->block_size[k] = taps.schedule.size[k];
  for (int k = 0; k < 3; k++) out->block_count[k] = taps.schedule.count[k];
  out->block_count[3] = taps.schedule.blocks_per_xcd - (taps.schedule.count[0] + taps.schedule.count[1] + taps.schedule.count[2]);
  if (out->streams)
    for (size_t i = 0; i < n; i++) {
      const FpStream &m = taps.streams[i];
      out->streams[i] = NeedleHipStageStream{m.frames, m.frame_base, m.pair_base, m.kept, m.kept_base, m.tile_base};
    }
  auto download = [](auto *dst, const auto *src, uint64_t count) -> Status {
    if (dst && count) NEEDLE_HIP_TRY(hipMemcpy(dst, src, count * sizeof(*dst), hipMemcpyDeviceToHost));
    return Status::Ok();
  };
  if (!(s = download(out->first_chroma, taps.first_chroma.ptr, taps.frames * kBands)).ok() ||
      !(s = download(out->energy, taps.energy.ptr, taps.frames * stft::kEnergyParts)).ok() ||
      !(s = download(out->final_chroma, taps.final_chroma.ptr, taps.frames * kBands)).ok() ||
      !(s = download(out->first_items, taps.first_items.ptr, taps.kept)).ok() || !(s = download(out->items, d_items.ptr, taps.kept)).ok())
    return s;
  // the two lists as counts per item and per chunk: 1 where listed, and more than 1 would be a double listing
  std::vector<uint32_t> ctl(taps.ctl_words), chunk_list(taps.nchunks);
  std::vector<CertItem> item_list(taps.kept);
  if (!(s = download(ctl.data(), taps.ctl.ptr, taps.ctl_words)).ok() || !(s = download(chunk_list.data(), taps.chunk_list.ptr, taps.nchunks)).ok() ||
      !(s = download(item_list.data(), taps.item_list.ptr, taps.kept)).ok())
    return s;
  const CertWork *work = CertLayout::work(ctl.data());
  const uint32_t *bitmap = CertLayout::bitmap(ctl.data());
  if (work->item_count > taps.kept || work->chunk_count > taps.nchunks)
    return Status::Make(NeedleError_Unknown, "fingerprint: the certification listed more items or chunks than there are");
  out->items_listed = work->item_count, out->chunks_listed = work->chunk_count;
  std::vector<uint8_t> per_item(taps.kept, 0), per_chunk(taps.nchunks, 0);
  for (uint32_t i = 0; i < work->item_count; i++) {
    if (item_list[i].out >= taps.kept) return Status::Make(NeedleError_Unknown, "fingerprint: a listed item lies outside the batch");
    if (per_item[item_list[i].out] < 255) per_item[item_list[i].out]++;
  }
  for (uint32_t i = 0; i < work->chunk_count; i++) {
    if (chunk_list[i] >= taps.nchunks) return Status::Make(NeedleError_Unknown, "fingerprint: a listed chunk lies outside the batch");
    if (per_chunk[chunk_list[i]] < 255) per_chunk[chunk_list[i]]++;
  }
  for (uint64_t c = 0; c < taps.nchunks; c++)
    if (((bitmap[c >> 5] >> (c & 31u)) & 1u) != (per_chunk[c] ? 1u : 0u))
      return Status::Make(NeedleError_Unknown, "fingerprint: the chunk bitmap and the chunk list disagree");
  if (out->item_listed && taps.kept) std::memcpy(out->item_listed, per_item.data(), taps.kept);
  if (out->chunk_listed && taps.nchunks) std::memcpy(out->chunk_listed, per_chunk.data(), taps.nchunks);
  return Status::Ok();
}

// {items fingerprinted, items recomputed in f64, chunks of frame pairs, chunks recomputed} since the last reset, on the
// current device; waits for the library stream.
Status gpu_fingerprint_cert_stats(uint64_t out[4], bool reset) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  Status s = ensure_device();
  if (!s.ok()) return s;
  FpWorkspace *ws = workspace();
  CertStats host{0, 0};
  hipStream_t stream = library_stream();
  if (ws->stats) {
    NEEDLE_HIP_TRY(hipMemcpyAsync(&host, ws->stats, sizeof(host), hipMemcpyDeviceToHost, stream));
    if (reset) NEEDLE_HIP_TRY(hipMemsetAsync(ws->stats, 0, sizeof(CertStats), stream));
    NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  }
  out[0] = ws->items_total;
  out[1] = host.items_recomputed;
  out[2] = ws->chunks_total;
  out[3] = host.chunks_recomputed;
  if (reset) ws->items_total = ws->chunks_total = 0;
  return Status::Ok();
}

// One feed of the streaming fingerprinter (feeder.hip) over all its lanes.  Two stream tables instead of one (plan_feed):
// the first pass sees the NEW frame pairs only and writes their rows behind the rows carried from earlier feeds;
// certification, recomputation and fix-up see carried + new frames.  The recomputation writes its f64 rows into
// `d_chroma64`, a buffer of its own with the same row numbering, and the fix-up reads them there: every frame of a listed
// item is in a listed chunk, and d_chroma keeps the first pass's rows for the next feed's certification.  Same kernels,
// same arithmetic, same pairs as gpu_fingerprint_device on the whole stream.
Status gpu_fingerprint_feed_device(const int16_t *d_pcm, const std::vector<FeedLane> &lanes, int channels, uint32_t step,
                                   double *d_chroma, float *d_energy, double *d_chroma64, uint32_t *d_items,
                                   const FeedAudit *audit) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  FpTables tab;
  Status s = begin_call(channels, step, &tab);
  if (!s.ok()) return s;
  hipStream_t stream = library_stream();
  FpWorkspace *ws = workspace();
  const Job job{tab, d_pcm, channels, step, tile_items(step), d_items, stream};
  FeedPlan plan;
  if (!(s = plan_feed(lanes, channels, step, job.items_per_tile, &plan)).ok()) return s;
  if (plan.pairs1 == 0 && plan.kept == 0) return Status::Ok();
  if (plan.pairs1 > 0x7FFFFFF0ull || plan.pairs2 > 0x7FFFFFF0ull) return Status::Make(NeedleError_InvalidArgument, "fingerprint: feed too large");
  if (audit && f64_mode()) return Status::Make(NeedleError_InvalidArgument, "fingerprint: NEEDLE_HIP_STFT=f64 has no first pass to audit");
  const uint64_t cus = (uint64_t)device_cu_count();
  const size_t streams2 = plan.second.size();
  if (audit && streams2) {  // the lanes of `second`, right behind its last stream (audit_items_kernel<PHASED>)
    constexpr size_t per = sizeof(FpStream) / sizeof(uint32_t);
    plan.second.resize(streams2 + (streams2 + per - 1) / per, FpStream{});
    std::memcpy(static_cast<void *>(plan.second.data() + streams2), plan.second_lane.data(), streams2 * sizeof(uint32_t));
  }
  if (!plan.first.empty() && !(s = ws->feed_first.upload.put(&ws->feed_first.streams, &ws->feed_first.stage, plan.first, stream)).ok()) return s;
  if (!plan.second.empty() && !(s = ws->feed_second.upload.put(&ws->feed_second.streams, &ws->feed_second.stage, plan.second, stream)).ok()) return s;
  const Table first{ws->feed_first.streams.ptr, (int)plan.first.size(), plan.pairs1};
  const Table second{ws->feed_second.streams.ptr, (int)streams2, plan.pairs2};
  // a feed is a short launch: every slot of the device gets one workgroup, of at most kPairsPerBlock pairs
  auto pairs_per_slot = [&](uint64_t slots) {
    return (uint32_t)std::min<uint64_t>(kPairsPerBlock, std::max<uint64_t>(1, (plan.pairs1 + slots - 1) / slots));
  };
  if (f64_mode()) return enqueue_f64(job, F64Chain{first, pairs_per_slot(2 * cus), d_chroma, second, plan.tiles, true, true});
  const CertLayout layout(plan.pairs2);
  if (!(s = ws->cert.reserve(layout, plan.kept, 0)).ok()) return s;
  const uint32_t ppb = pairs_per_slot((uint64_t)kStft32WavesPerSimd * cus);
  const FirstPass pass{first, stft32_schedule(plan.pairs1, ppb, 0, false), d_chroma, d_energy, ws->cert.ctl.ptr,
                       (uint32_t)layout.ctl_words, stream, nullptr, true};
  bool zeroed = false;
  s = enqueue_certified(job, ws, CertChain{pass, second, plan.tiles, plan.kept, true, d_chroma64, &ws->cert,
                                           (uint32_t)std::min<uint64_t>(2 * cus, layout.nchunks), false, nullptr, plan.chunks1}, &zeroed);
  if (!s.ok() || !audit) return s;
  static_assert(sizeof(AuditCounts) == kFeedAuditWords * sizeof(uint64_t), "a feeder lane's audit counts are kFeedAuditWords words");
  // The audit that travels with the stream: every new pair through the f64 kernel once, into the audit's own rows (not
  // d_chroma64: that holds the listed chunks alone), then every new kept item examined as the one-shot audit examines it.
  if (plan.pairs1) {
    KernelTimer timer("audit_stft");
    if (!(s = enqueue_f64(job, F64Chain{first, pairs_per_slot(2 * cus), audit->rows64, second, 0, true, false})).ok()) return s;
  }
  if (plan.tiles) {
    KernelTimer timer("audit_items");
    hipLaunchKernelGGL(audit_items_kernel<true>, dim3((uint32_t)plan.tiles), dim3(64), 0, stream, d_chroma, d_energy, audit->rows64,
                       second.streams, second.n, tab.thr, step, job.items_per_tile, d_items, (uint32_t)plan.tiles, cert_k(),
                       reinterpret_cast<AuditCounts *>(audit->counts));
    NEEDLE_HIP_TRY(hipGetLastError());
  }
  return Status::Ok();
}

bool gpu_fingerprint_f64_mode() { return f64_mode(); }

// Audit (include/needle_hip.h needle_hip_fingerprint_audit_device): both transforms over the same resident PCM, every
// kept item compared on the device.  out = {items, accepted by the first pass, accepted items whose f32 bits are not the
// f64 item, items of d_items that are not the f64 item}; *max_ratio = max |log v32 - log v64| / S over accepted items.
Status gpu_fingerprint_audit_device(const int16_t *d_pcm, const std::vector<StreamSpan> &spans, int channels, uint32_t step,
                                    const uint32_t *d_items, uint64_t out[4], double *max_ratio, double *max_sigma) {
  std::lock_guard<std::recursive_mutex> gpu_lock(gpu_mutex());
  FpTables tab;
  Status s = begin_call(channels, step, &tab);
  if (!s.ok()) return s;
  hipStream_t stream = library_stream();
  // buffers of its own, freed on return: an audit must not disturb the workspaces of jobs in flight
  DeviceBuffer<double> chroma32, chroma64;
  DeviceBuffer<float> energy;
  DeviceBuffer<uint32_t> ctl;  // the first pass zeroes a CertWork's worth of it; nothing reads it
  DeviceBuffer<FpStream> d_streams;
  DeviceBuffer<AuditCounts> d_counts;
  if (!(s = d_counts.reserve(1)).ok() || !(s = ctl.reserve(64)).ok()) return s;
  NEEDLE_HIP_TRY(hipMemsetAsync(d_counts.ptr, 0, sizeof(AuditCounts), stream));
  const float k = cert_k();
  const uint64_t max_frames = max_frames_per_chunk(4u << 20);
  const Job job{tab, d_pcm, channels, step, tile_items(step), nullptr, stream};  // (nothing here writes items)
  size_t begin = 0;
  while (begin < spans.size()) {
    ChunkPlan plan;
    if (!(s = plan_chunk(spans, begin, channels, step, job.items_per_tile, max_frames, &plan)).ok()) return s;
    begin = plan.end;
    if (plan.frames == 0 || plan.tiles == 0) continue;
    if (!(s = chroma32.reserve(plan.frames * kBands)).ok() || !(s = chroma64.reserve(plan.frames * kBands)).ok() ||
        !(s = energy.reserve(plan.frames * stft::kEnergyParts)).ok() || !(s = d_streams.reserve(plan.streams.size())).ok())
      return s;
    NEEDLE_HIP_TRY(hipStreamSynchronize(stream));  // the previous chunk still reads d_streams; the plan is pageable
    NEEDLE_HIP_TRY(hipMemcpyAsync(d_streams.ptr, plan.streams.data(), plan.streams.size() * sizeof(FpStream), hipMemcpyHostToDevice, stream));
    NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
    const Table table{d_streams.ptr, (int)plan.streams.size(), plan.pairs};
    if (!(s = enqueue_first_pass(job, FirstPass{table, stft32_schedule(plan.pairs, kPairsPerBlock, 0, false), chroma32.ptr, energy.ptr,
                                                ctl.ptr, (uint32_t)(sizeof(CertWork) / 4), stream, nullptr, false})).ok() ||
        !(s = enqueue_f64(job, F64Chain{table, (uint32_t)kPairsPerBlock, chroma64.ptr, table, 0, false, false})).ok())
      return s;
    hipLaunchKernelGGL(audit_items_kernel<false>, dim3((uint32_t)plan.tiles), dim3(64), 0, stream, chroma32.ptr, energy.ptr, chroma64.ptr,
                       table.streams, table.n, tab.thr, step, job.items_per_tile, d_items, (uint32_t)plan.tiles, k, d_counts.ptr);
    NEEDLE_HIP_TRY(hipGetLastError());
  }
  AuditCounts host;
  NEEDLE_HIP_TRY(hipMemcpyAsync(&host, d_counts.ptr, sizeof(host), hipMemcpyDeviceToHost, stream));
  NEEDLE_HIP_TRY(hipStreamSynchronize(stream));
  out[0] = host.items;
  out[1] = host.accepted;
  out[2] = host.accepted_wrong;
  out[3] = host.final_wrong;
  double ratio = 0.0, sigma = 0.0;
  std::memcpy(&ratio, &host.max_ratio_bits, sizeof(double));
  std::memcpy(&sigma, &host.max_sigma_bits, sizeof(double));
  if (max_ratio) *max_ratio = ratio;
  if (max_sigma) *max_sigma = sigma;
  return Status::Ok();
}

}  // namespace needle
