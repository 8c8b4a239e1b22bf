// Host-side check of needle_amd/csrc/job_plan.h: the plan and the verdict of a library job for synthetic shapes, switches,
// histories and counts that take every branch (tests/test_job_plan_cpu.py lists the families).  For every case and EVERY
// RANK of its world it asserts what the executor (library.cpp) and the transport (comm.h) rely on, independently of any
// recorded output, and drives plan_job -> judge -> plan_job with the counts held constant (the scan is deterministic)
// until the job is done.  Beside them it runs the expressions as they stood in library.cpp before (namespace `before`) and
// asserts that plan, verdict and history agree.  It prints one line per case -- the plan of the first attempt, the form
// of every attempt, the verdicts, the history left -- which the test compares with tests/golden/job_plans.txt.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../needle_amd/csrc/job_plan.h"

using namespace needle;

namespace {

struct Case {
  std::string name;
  JobShape shape;
  JobSwitches sw;
  JobHistory hist;
  std::vector<uint32_t> slab;    // per rank: runs found (default below)
  std::vector<uint32_t> matrix;  // [W][W]: runs rank r directs to rank q (default below)
};

int g_failed = 0;
#define CHECK(cond, ...)                                \
  do {                                                  \
    if (!(cond)) {                                      \
      std::printf("%s: INVARIANT ", c.name.c_str());    \
      std::printf(__VA_ARGS__);                         \
      std::printf(" (%s)\n", #cond);                    \
      g_failed++;                                       \
    }                                                   \
  } while (0)

struct Digest {
  uint64_t h = 1469598103934665603ull;
  void add(uint64_t v) {
    for (int k = 0; k < 8; k++) {
      h ^= (v >> (8 * k)) & 0xff;
      h *= 1099511628211ull;
    }
  }
  template <class T>
  void add(const std::vector<T> &v) {
    add(v.size());
    for (const T &x : v) add((uint64_t)x);
  }
};

JobHook on(int v) { return JobHook{true, v}; }
uint32_t ragged(size_t r, size_t q) { return (uint32_t)(10 + 37 * r + 5 * q + (r == q ? 100 : 0)); }
std::vector<uint32_t> ragged_matrix(int world, uint32_t scale = 1) {
  std::vector<uint32_t> m;
  for (size_t r = 0; r < (size_t)world; r++)
    for (size_t q = 0; q < (size_t)world; q++) m.push_back(ragged(r, q) * scale);
  return m;
}

// form, sizes, cap matrix, max_block_bytes: what must not depend on the rank
bool same_everywhere(const JobPlan &a, const JobPlan &b) {
  return a.device_epilogue == b.device_epilogue && a.sharded == b.sharded && a.shape_fixed == b.shape_fixed &&
         a.slab_runs == b.slab_runs && a.head_runs == b.head_runs && a.pinned_bytes == b.pinned_bytes &&
         a.directed.wanted == b.directed.wanted && a.directed.sized == b.directed.sized && a.directed.refused == b.directed.refused &&
         a.directed.cap_consumed == b.directed.cap_consumed && a.directed.cap == b.directed.cap &&
         a.directed.max_block_bytes == b.directed.max_block_bytes && a.segments.kind == b.segments.kind;
}

void check_plans(const Case &c, const std::vector<JobPlan> &plans) {
  const int world = c.shape.world;
  const size_t W = (size_t)world;
  size_t pair_at = 0, video_at = 0;
  for (size_t q = 0; q < W; q++) {
    const JobPlan &p = plans[q];
    const DirectedPlan &d = p.directed;
    // 1. the same form, sizes, caps and largest block on all ranks; only the injected failure differs
    CHECK(same_everywhere(p, plans[0]), "rank %zu plans another job than rank 0", q);
    CHECK(p.inject_epilogue_failure ==
              (p.device_epilogue && c.sw.test_epilogue_fail_rank.set && c.sw.test_epilogue_fail_rank.value == (int)q),
          "rank %zu: injected failure", q);
    CHECK(!p.sharded || p.device_epilogue, "rank %zu: sharded is decided at the enqueue for the device form only", q);
    CHECK(p.shape_fixed == p.device_epilogue, "rank %zu", q);
    CHECK(!d.sized || d.wanted, "rank %zu", q);
    CHECK(!d.wanted || (world > 1 && world <= 64 && p.device_epilogue && p.sharded), "rank %zu: directed without its form", q);
    // 5. the head fits the slab, the pinned buffer the heads of all ranks
    CHECK(p.head_runs <= p.slab_runs && p.head_runs % 4 == 0 && p.slab_runs % 4 == 0 && p.slab_runs >= 4, "rank %zu: %u / %u", q,
          p.head_runs, p.slab_runs);
    CHECK(p.pinned_bytes >= p.head_bytes() * W, "rank %zu", q);
    CHECK(p.head_bytes() % 4 == 0, "rank %zu: the gather of heads", q);  // 4.
    // 7. pair ranges and video ranges tile their totals
    CHECK(p.pair_first == pair_at, "rank %zu: pairs start at %zu, not %zu", q, p.pair_first, pair_at);
    pair_at += p.pair_count;
    if (p.sharded) {
      CHECK(p.video_first == video_at, "rank %zu: videos start at %zu, not %zu", q, p.video_first, video_at);
      video_at += p.video_count;
    } else {
      CHECK(p.video_first == 0 && p.video_count == c.shape.n, "rank %zu: all videos", q);
    }
    // 6. the segment capacities sum to max_runs
    const SegmentLayout &s = p.segments;
    uint64_t sum = 0;
    for (size_t r = 0; r < W; r++) sum += s.capacity ? s.capacity : (s.capacities.empty() ? 0 : s.capacities[r]);
    CHECK(sum == s.max_runs, "rank %zu: segments hold %llu runs, max_runs %llu", q, (unsigned long long)sum, (unsigned long long)s.max_runs);
    CHECK((s.kind == SegmentKind::Blocks) == d.sized && (s.kind == SegmentKind::Slab) == (world == 1), "rank %zu: segment kind", q);
    CHECK(s.kind != SegmentKind::Blocks || (s.capacity == 0 && s.capacities.size() == W), "rank %zu", q);
    if (!d.wanted) continue;
    CHECK(count_matrix_bytes(world) % 16 == 0 && count_words(world) >= W + 1, "rank %zu: count rows", q);  // 4.
    CHECK(d.cap.size() == W * W && d.send_off.size() == W && d.send_bytes.size() == W && d.send_capacity.size() == W &&
              d.recv_off.size() == W && d.recv_bytes.size() == W,
          "rank %zu: sizes of the directed plan", q);
    // 3. + 4. blocks tile [0, total) in rank order; every size and offset is a multiple of 4
    size_t at = 0, rat = 0, largest = 0;
    for (size_t r = 0; r < W; r++) {
      CHECK(d.send_off[r] == at && d.send_bytes[r] == slab_bytes(d.send_capacity[r]) && d.send_capacity[r] == d.cap[q * W + r],
            "rank %zu: send block %zu", q, r);
      CHECK(d.send_off[r] % 4 == 0 && d.send_bytes[r] % 4 == 0, "rank %zu: send block %zu", q, r);
      at += d.send_bytes[r];
      if (d.sized) {
        CHECK(d.recv_off[r] == rat && d.recv_off[r] % 4 == 0 && d.recv_bytes[r] % 4 == 0, "rank %zu: receive block %zu", q, r);
        // 2. what rank q receives from rank r is what rank r sends to rank q
        CHECK(d.recv_bytes[r] == plans[r].directed.send_bytes[q], "rank %zu <- %zu: %zu bytes expected, %zu sent", q, r, d.recv_bytes[r],
              plans[r].directed.send_bytes[q]);
        CHECK(p.segments.capacities[r] == plans[r].directed.send_capacity[q], "rank %zu <- %zu: segment capacity", q, r);
        rat += d.recv_bytes[r];
      }
      largest = std::max(largest, plans[r].directed.send_total ? *std::max_element(plans[r].directed.send_bytes.begin(), plans[r].directed.send_bytes.end()) : 0);
    }
    CHECK(at == d.send_total && rat == d.recv_total, "rank %zu: totals", q);
    CHECK(d.max_block_bytes == largest && d.max_block_bytes % 4 == 0, "rank %zu: largest block %zu, %zu planned", q, largest, d.max_block_bytes);
    CHECK(d.refused == (d.send_total >= 0xFFFFFFF0ull), "rank %zu", q);
    CHECK(d.refused || d.send_off[W - 1] <= 0xffffffffull, "rank %zu: 32-bit offsets", q);
  }
  CHECK(pair_at == job_pairs(c.shape.n), "pair ranges cover %zu of %llu", pair_at, (unsigned long long)job_pairs(c.shape.n));
  CHECK(!plans[0].sharded || video_at == c.shape.n, "video ranges cover %zu of %zu", video_at, c.shape.n);
}


// ---- The expressions as they stood in library.cpp before job_plan.h existed (job_begin's first slab, job_buffers,
// job_search_and_gather, the loop of job_end), copied with their names and their order; getenv(NAME) became a JobHook (set =
// the variable exists, value = atoi of it), `lib->` and `j.` became the two structs below, the HIP and comm calls are left
// out.  Every case runs them beside plan_job / judge for every rank and attempt and asserts that the two agree: the recorded
// lines therefore hold for the old expressions as much as for the new ones.
namespace before {
constexpr size_t kSlabHeader = 32;
uint32_t round_up4(uint64_t v) { return (uint32_t)std::min<uint64_t>((v + 3) & ~(uint64_t)3, 0xfffffffcu); }
size_t pair_count(size_t n) { return n < 2 ? 0 : n * (n - 1) / 2; }
struct Lib {
  size_t n = 0, regions = 1;
  uint32_t slab_runs = 0, last_max_count = 0;
  std::vector<uint32_t> dir_counts;
  int dir_world = 0;
  bool dir_unsupported = false, dir_cap_forced = false;
};
struct Job {
  uint32_t slab_runs = 0, head_runs = 0;
  bool device_epilogue = false, sharded = false, shape_fixed = false, counted = false, directed = false, refused = false;
  std::vector<uint32_t> cap, all_caps;
  std::vector<size_t> send_off, send_bytes, recv_off, recv_bytes;
  size_t largest = 0, send_total = 0, recv_total = 0, pfirst = 0, pcount = 0, v0 = 0, vcount = 0;
  size_t slab_bytes() const { return kSlabHeader + (size_t)slab_runs * sizeof(NeedleHipRun); }
  size_t head_bytes() const { return kSlabHeader + (size_t)head_runs * sizeof(NeedleHipRun); }
};
void job_begin_slab(Lib *lib, const JobSwitches &env, int world) {
  if (lib->slab_runs == 0 && env.slab_runs.set) lib->slab_runs = round_up4((uint64_t)std::max(4, env.slab_runs.value));
  if (lib->slab_runs == 0)
    lib->slab_runs = round_up4(std::max<uint64_t>(1024, 4 * (uint64_t)shard_block(pair_count(lib->n), world) * lib->regions));
}
void job_buffers(Lib *lib, Job &j, const JobSwitches &env, int world) {
  j.slab_runs = lib->slab_runs;
  uint32_t head = lib->last_max_count ? round_up4((uint64_t)lib->last_max_count + lib->last_max_count / 8 + 64) : 4096u;
  const bool forced = lib->last_max_count ? false : env.head_runs.set;
  if (forced) head = round_up4((uint64_t)std::max(4, env.head_runs.value));
  head = std::min(head, j.slab_runs);
  if (!forced && j.slab_bytes() * (size_t)world <= (1u << 20)) head = j.slab_runs;
  j.head_runs = head;
}
bool device_epilogue_wanted(const Lib *lib, const JobSwitches &env, size_t comparator_regions) {
  if (env.device_epilogue.set) return env.device_epilogue.value != 0;
  return (uint64_t)pair_count(lib->n) * comparator_regions >= kDeviceEpiloguePairs || lib->last_max_count >= kDeviceEpilogueRuns;
}
void job_search_and_gather(Lib *lib, Job &j, const JobSwitches &env, size_t Rc, int world, int rank) {
  shard_range(pair_count(lib->n), world, rank, &j.pfirst, &j.pcount);
  j.device_epilogue = device_epilogue_wanted(lib, env, Rc) && lib->n >= 2;
  j.shape_fixed = j.device_epilogue;
  if (j.device_epilogue) {
    uint64_t shard_from = 1u << 16;
    if (env.shard_epilogue_pairs.set) shard_from = (uint64_t)std::max(1, env.shard_epilogue_pairs.value);
    j.sharded = world > 1 && (env.shard_epilogue.set ? env.shard_epilogue.value != 0 : (uint64_t)pair_count(lib->n) * Rc >= shard_from);
  }
  j.counted = j.directed = j.refused = false;
  j.cap.clear();
  j.all_caps.clear();
  const bool want_directed = world > 1 && world <= 64 && j.device_epilogue && j.sharded && !lib->dir_unsupported &&
                             !(env.directed_runs.set && env.directed_runs.value == 0);
  j.recv_off.assign((size_t)world, 0), j.recv_bytes.assign((size_t)world, 0);
  j.send_off.clear(), j.send_bytes.clear();
  j.largest = j.send_total = j.recv_total = 0;
  if (want_directed) {
    const size_t W = (size_t)world;
    const bool have = lib->dir_world == world && lib->dir_counts.size() == W * W;
    std::vector<uint32_t> cap(W * W, 0u);
    if (have)
      for (size_t k = 0; k < W * W; k++) cap[k] = round_up4((uint64_t)lib->dir_counts[k] + lib->dir_counts[k] / 8 + 64);
    if (env.test_directed_cap.set)
      if (have && !lib->dir_cap_forced) {
        std::fill(cap.begin(), cap.end(), round_up4((uint64_t)std::max(4, env.test_directed_cap.value)));
        lib->dir_cap_forced = true;
      }
    j.send_off.resize(W), j.send_bytes.resize(W);
    size_t off = 0, largest = 0;
    for (size_t q = 0; q < W; q++) {
      j.send_off[q] = off;
      j.send_bytes[q] = kSlabHeader + (size_t)cap[(size_t)rank * W + q] * sizeof(NeedleHipRun);
      off += j.send_bytes[q];
    }
    for (size_t k = 0; k < W * W; k++) largest = std::max(largest, kSlabHeader + (size_t)cap[k] * sizeof(NeedleHipRun));
    j.largest = largest, j.send_total = off, j.all_caps = cap;
    if (off >= 0xFFFFFFF0ull) {
      j.refused = true;
      return;
    }
    j.counted = true;
    if (have) {
      size_t roff = 0;
      for (size_t r = 0; r < W; r++) {
        j.recv_off[r] = roff;
        j.recv_bytes[r] = kSlabHeader + (size_t)cap[r * W + (size_t)rank] * sizeof(NeedleHipRun);
        roff += j.recv_bytes[r];
      }
      j.recv_total = roff;
      j.directed = true;
      j.cap = cap;
    }
  }
  j.v0 = 0, j.vcount = lib->n;
  if (j.device_epilogue && j.sharded) shard_range(lib->n, world, rank, &j.v0, &j.vcount);
}
// one turn of job_end's loop: true = the job was repeated (comm_bytes[3]++), false = break.  `slab` = every rank's count,
// `m` = the count matrix [W][W] (what host_counts held, without its first column)
bool job_end_turn(Lib *lib, Job &j, const JobSwitches &env, size_t Rc, int world, int rank, const std::vector<uint32_t> &slab,
                  const std::vector<uint32_t> &m) {
  const size_t W = (size_t)world;
  auto take_matrix = [&]() {
    lib->dir_counts = m;
    lib->dir_world = world;
  };
  uint32_t most = 0;
  for (size_t r = 0; r < W; r++) most = std::max(most, slab[r]);
  if (j.directed) {
    if (most <= j.slab_runs) {
      bool fits = true;
      for (size_t r = 0; r < W && fits; r++)
        for (size_t q = 0; q < W && fits; q++) fits = m[r * W + q] <= j.cap[r * W + q];
      take_matrix();
      lib->last_max_count = most;
      if (fits) return false;
      job_search_and_gather(lib, j, env, Rc, world, rank);
      return true;
    }
  } else {
    if (most <= j.slab_runs && (world == 1 || most <= j.head_runs)) {
      lib->last_max_count = most;
      if (j.counted) take_matrix();
      return false;
    }
    if (most <= j.slab_runs) {
      lib->last_max_count = most;
      job_buffers(lib, j, env, world);
      job_search_and_gather(lib, j, env, Rc, world, rank);
      return true;
    }
  }
  lib->slab_runs = round_up4((uint64_t)most + most / 4 + 64);
  lib->last_max_count = most;
  lib->dir_counts.clear();
  job_buffers(lib, j, env, world);
  job_search_and_gather(lib, j, env, Rc, world, rank);
  return true;
}
bool shard_epilogue(const JobHook &env, size_t total_runs) {
  if (env.set) return env.value != 0;
  return total_runs >= (1u << 17);
}
}  // namespace before

// the plan of one rank's attempt against what the old expressions arrive at for it
void check_against_before(const Case &c, const JobPlan &p, const before::Job &j, const before::Lib &lib) {
  const DirectedPlan &d = p.directed;
  CHECK(p.slab_runs == j.slab_runs && p.head_runs == j.head_runs && p.slab_runs == lib.slab_runs, "rank %d: sizes %u / %u, before %u / %u",
        p.shape.rank, p.slab_runs, p.head_runs, j.slab_runs, j.head_runs);
  CHECK(p.device_epilogue == j.device_epilogue && p.shape_fixed == j.shape_fixed && (!j.device_epilogue || p.sharded == j.sharded),
        "rank %d: form", p.shape.rank);
  CHECK(p.pair_first == j.pfirst && p.pair_count == j.pcount && (j.refused || (p.video_first == j.v0 && p.video_count == j.vcount)), "rank %d: ranges",
        p.shape.rank);  // (a refused job never came to its epilogue)
  CHECK(d.refused == j.refused && d.wanted == (j.counted || j.refused) && (d.sized && !d.refused) == j.directed, "rank %d: directed", p.shape.rank);
  CHECK(d.cap == j.all_caps && d.send_off == j.send_off && d.send_bytes == j.send_bytes && d.send_total == j.send_total &&
            d.max_block_bytes == j.largest,
        "rank %d: send side", p.shape.rank);
  if (!d.refused)
    CHECK((d.wanted ? d.recv_off == j.recv_off && d.recv_bytes == j.recv_bytes : true) && d.recv_total == j.recv_total, "rank %d: receive side",
          p.shape.rank);
  CHECK(p.pinned_bytes == j.head_bytes() * (size_t)p.shape.world, "rank %d: pinned bytes", p.shape.rank);
}
void check_history(const Case &c, const JobHistory &h, const before::Lib &lib) {
  CHECK(h.slab_runs == lib.slab_runs && h.last_max_count == lib.last_max_count && h.dir_counts == lib.dir_counts && h.dir_world == lib.dir_world &&
            h.dir_cap_forced == lib.dir_cap_forced,
        "the history differs from what the old expressions leave: slab %u / %u, last %u / %u", h.slab_runs, lib.slab_runs, h.last_max_count,
        lib.last_max_count);
}

std::vector<JobPlan> plans_of(const Case &c, const JobHistory &h, uint32_t keep_head) {
  std::vector<JobPlan> plans;
  for (int r = 0; r < c.shape.world; r++) {
    JobShape s = c.shape;
    s.rank = r;
    plans.push_back(plan_job(s, c.sw, h, keep_head));
  }
  return plans;
}

const char *name_of(JobNext n) {
  return n == JobNext::Done ? "done" : n == JobNext::GrowHead ? "head" : n == JobNext::GrowBlocks ? "blocks" : "slab";
}

void run(Case c) {
  const int world = c.shape.world;
  const size_t W = (size_t)world;
  if (c.slab.empty())
    for (size_t r = 0; r < W; r++) c.slab.push_back((uint32_t)(100 + r));
  if (c.matrix.empty()) c.matrix = ragged_matrix(world);
  JobHistory hist = c.hist;
  // the old expressions' state, one library and one job slot per rank
  std::vector<before::Lib> libs(W);
  std::vector<before::Job> jobs(W);
  for (size_t r = 0; r < W; r++) {
    before::Lib &l = libs[r];
    l.n = c.shape.n, l.regions = c.shape.arena_regions;
    l.slab_runs = hist.slab_runs, l.last_max_count = hist.last_max_count, l.dir_counts = hist.dir_counts, l.dir_world = hist.dir_world;
    l.dir_unsupported = hist.dir_unsupported, l.dir_cap_forced = hist.dir_cap_forced;
    before::job_begin_slab(&l, c.sw, world);
    before::job_buffers(&l, jobs[r], c.sw, world);
    before::job_search_and_gather(&l, jobs[r], c.sw, c.shape.comparator_regions, world, (int)r);
  }
  std::string verdicts;
  int repeats = 0;
  bool done = false;
  uint32_t keep_head = 0;
  for (int attempt = 0; attempt < 6 && !done; attempt++) {
    const std::vector<JobPlan> plans = plans_of(c, hist, keep_head);
    check_plans(c, plans);
    const JobPlan &p = plans[0];
    if (attempt == 0) {
      Digest sides;  // every rank's send and receive side
      for (const JobPlan &q : plans) {
        sides.add(q.pair_first), sides.add(q.pair_count), sides.add(q.video_first), sides.add(q.video_count);
        sides.add(q.directed.send_off), sides.add(q.directed.send_bytes), sides.add(q.directed.recv_off), sides.add(q.directed.recv_bytes);
        sides.add(q.directed.send_capacity), sides.add(q.segments.capacities), sides.add(q.segments.max_runs);
      }
      Digest caps;
      caps.add(p.directed.cap);
      std::printf("%s: n=%zu Ra=%zu Rc=%zu W=%d | device=%d sharded=%d fixed=%d wanted=%d sized=%d refused=%d cap_used=%d slab=%u head=%u pinned=%zu "
                  "blk=%zu seg=%d/%u/%llu pairs0=%zu+%zu videos0=%zu+%zu caps=%016llx sides=%016llx |",
                  c.name.c_str(), c.shape.n, c.shape.arena_regions, c.shape.comparator_regions, world, p.device_epilogue, p.sharded, p.shape_fixed,
                  p.directed.wanted, p.directed.sized, p.directed.refused, p.directed.cap_consumed, p.slab_runs, p.head_runs, p.pinned_bytes,
                  p.directed.max_block_bytes, (int)p.segments.kind, p.segments.capacity, (unsigned long long)p.segments.max_runs, p.pair_first,
                  p.pair_count, p.video_first, p.video_count, (unsigned long long)caps.h, (unsigned long long)sides.h);
    }
    // what the caller writes back when it executes the plan
    hist.slab_runs = p.slab_runs;
    if (p.directed.cap_consumed) hist.dir_cap_forced = true;
    for (size_t r = 0; r < W; r++) check_against_before(c, plans[r], jobs[r], libs[r]);
    check_history(c, hist, libs[0]);
    // every attempt's form, so that a form or a head frozen -- or not -- at a repeat shows in the line
    char form[96];
    std::snprintf(form, sizeof form, " [device=%d sharded=%d sized=%d slab=%u head=%u]", p.device_epilogue, p.sharded, p.directed.sized, p.slab_runs,
                  p.head_runs);
    verdicts += form;
    if (p.directed.refused) {  // the job fails on every rank, before any transfer
      verdicts += " refused";
      break;
    }
    JobCounts counts;
    counts.directed = p.directed.sized;
    counts.slab = c.slab;
    if (p.directed.wanted) counts.directed_to = c.matrix;
    // 8. every rank draws the same verdict from the same counts
    const JobVerdict v = judge(p, counts, hist);
    for (const JobPlan &q : plans) {
      const JobVerdict vq = judge(q, counts, hist);
      CHECK(vq.next == v.next && vq.most == v.most && vq.keep_head == v.keep_head && vq.history.slab_runs == v.history.slab_runs &&
                vq.history.last_max_count == v.history.last_max_count && vq.history.dir_counts == v.history.dir_counts &&
                vq.history.dir_world == v.history.dir_world,
            "rank %d draws another verdict", q.shape.rank);
    }
    for (size_t r = 0; r < W; r++) {
      const bool repeated = before::job_end_turn(&libs[r], jobs[r], c.sw, c.shape.comparator_regions, world, (int)r, c.slab, c.matrix);
      CHECK(repeated == (v.next != JobNext::Done), "rank %zu: the old loop %s", r, repeated ? "repeats" : "ends");
    }
    // what the verdict leaves of the matrix
    if (v.next == JobNext::GrowSlab) CHECK(v.history.dir_counts.empty(), "a slab overflow keeps a matrix counted over a clamped slab");
    if (v.next == JobNext::GrowHead) CHECK(v.history.dir_counts == hist.dir_counts, "a head overflow takes the matrix");
    if (v.next == JobNext::GrowBlocks || (v.next == JobNext::Done && p.directed.wanted))
      CHECK(v.history.dir_counts == c.matrix && v.history.dir_world == world, "the matrix is not taken");
    CHECK(v.keep_head == (v.next == JobNext::GrowBlocks ? p.head_runs : 0u), "keep_head %u", v.keep_head);
    verdicts += std::string(" ") + name_of(v.next);
    hist = v.history;
    keep_head = v.keep_head;
    done = v.next == JobNext::Done;
    if (done) {
      check_history(c, hist, libs[0]);
      break;
    }
    repeats++;
    // 9. after a "grow", the capacity that overflowed holds the count that overflowed it
    const JobPlan next = plan_job(c.shape, c.sw, hist, keep_head);
    if (v.next == JobNext::GrowSlab) {
      CHECK(next.slab_runs >= v.most, "slab %u after %u runs", next.slab_runs, v.most);
      CHECK(!next.directed.sized, "block sizes from a matrix that was cleared");
    }
    if (v.next == JobNext::GrowHead) CHECK(next.head_runs >= v.most || !(next.shape.world > 1), "head %u after %u runs", next.head_runs, v.most);
    if (v.next == JobNext::GrowBlocks) CHECK(next.head_runs == p.head_runs, "head %u after a block overflow, %u before", next.head_runs, p.head_runs);
    if (v.next == JobNext::GrowBlocks && next.directed.sized)
      for (size_t k = 0; k < W * W; k++) CHECK(next.directed.cap[k] >= c.matrix[k], "block %zu: %u after %u runs", k, next.directed.cap[k], c.matrix[k]);
  }
  CHECK(done || verdicts.find("refused") != std::string::npos, "the repeat loop does not end:%s", verdicts.c_str());
  Digest left;
  left.add(hist.dir_counts);
  std::printf("%s repeats=%d | slab=%u last=%u dir_world=%d dir=%016llx forced=%d\n", verdicts.c_str(), repeats, hist.slab_runs, hist.last_max_count,
              hist.dir_world, (unsigned long long)left.h, hist.dir_cap_forced);
}

Case base(const std::string &name, size_t n, int world, size_t Ra = 1, size_t Rc = 1) {
  Case c;
  c.name = name;
  c.shape.n = n;
  c.shape.world = world;
  c.shape.arena_regions = Ra;
  c.shape.comparator_regions = Rc;
  return c;
}

// a history as a library of this shape has it after one finished job that counted: sizes, and a ragged matrix
JobHistory after_one_job(int world, uint32_t slab, uint32_t last, uint32_t scale = 1) {
  JobHistory h;
  h.slab_runs = slab;
  h.last_max_count = last;
  h.dir_counts = ragged_matrix(world, scale);
  h.dir_world = world;
  return h;
}

}  // namespace

int main() {
  const int worlds[] = {1, 2, 3, 5, 8, 64, 65};
  // ---- form
  // pairs x comparator regions one below and at kDeviceEpiloguePairs (16 384): 181 videos have 16 290 pairs, 182 have 16 471;
  // 129 videos with endings 8 256 x 2 = 16 512, 128 videos 8 128 x 2 = 16 256
  for (size_t n : {181, 182})
    for (int w : {1, 2}) run(base("form/pairs", n, w));
  for (size_t n : {128, 129}) run(base("form/pairs-regions", n, 2, 2, 2));
  for (uint32_t last : {kDeviceEpilogueRuns - 1, kDeviceEpilogueRuns})
    for (int w : {1, 2}) {
      Case c = base("form/last-count", 28, w);
      c.hist.slab_runs = 1u << 16;
      c.hist.last_max_count = last;
      run(c);
    }
  for (size_t n : {1, 2})
    for (int w : {1, 2}) {
      Case c = base("form/n", n, w);
      c.sw.device_epilogue = on(1);
      c.sw.shard_epilogue = on(1);
      run(c);
    }
  for (int dev : {0, 1})
    for (int shard : {-1, 0, 1})
      for (int dir : {-1, 0, 1}) {
        Case c = base("form/switches", dev ? 28 : 400, 3);
        c.sw.device_epilogue = on(dev);
        if (shard >= 0) c.sw.shard_epilogue = on(shard);
        if (dir >= 0) c.sw.directed_runs = on(dir);
        c.hist = after_one_job(3, 4096, 200);
        run(c);
      }
  for (size_t n : {362, 363}) run(base("form/shard-threshold", n, 2));  // 65 341 and 65 703 pairs
  {
    Case c = base("form/shard-threshold-pairs", 182, 2);
    c.sw.shard_epilogue_pairs = on(1);
    run(c);
    c.sw.shard_epilogue_pairs = on(0);  // (clamped to 1)
    c.shape.n = 2;
    c.sw.device_epilogue = on(1);
    run(c);
  }
  for (int w : worlds) {
    Case c = base("form/world", 400, w);
    run(c);
    c.name = "form/world-history";
    c.hist = after_one_job(w, 65536, 300);
    run(c);
  }
  for (size_t Ra : {1, 2})
    for (size_t Rc : {1, 2})
      run(base("form/regions", 150, 2, Ra, Rc));
  for (int fail : {0, 1, 2}) {
    Case c = base("form/epilogue-fails-on-one-rank", 28, 3);
    c.sw.device_epilogue = on(1);
    c.sw.shard_epilogue = on(1);
    c.sw.test_epilogue_fail_rank = on(fail);
    c.hist = after_one_job(3, 4096, 200);
    run(c);
  }
  // ---- sizes
  for (size_t n : {7, 28, 400, 2000})
    for (int w : {1, 2, 8})
      for (size_t Ra : {1, 2}) run(base("sizes/first-job", n, w, Ra, 1));
  // the whole slab while all slabs are at most 1 MiB: 2 slabs of 21 844 runs are 1 048 576 bytes, of 21 848 more
  for (uint32_t slab : {21840u, 21844u, 21848u}) {
    Case c = base("sizes/one-mib", 28, 2);
    c.hist.slab_runs = slab;
    c.hist.last_max_count = 500;
    run(c);
  }
  for (int head : {1, 8, 4099, 1 << 20})
    for (uint32_t last : {0u, 50u}) {
      Case c = base("sizes/forced-head", 28, 2);
      c.sw.head_runs = on(head);
      c.hist.last_max_count = last;  // (a first head only)
      run(c);
    }
  for (int slab : {-5, 1, 8, 1001})
    for (uint32_t had : {0u, 2048u}) {
      Case c = base("sizes/forced-slab", 28, 2);
      c.sw.slab_runs = on(slab);
      c.hist.slab_runs = had;  // (a first slab only)
      c.slab = {40, 30};
      run(c);
    }
  for (uint32_t last : {0xe0000000u, 0xe38e38e0u, 0xfffffff0u, 0xffffffffu}) {
    Case c = base("sizes/round-up4-clamp", 28, 2);
    c.hist.slab_runs = 0xfffffffcu;
    c.hist.last_max_count = last;
    run(c);
  }
  for (uint32_t last : {1u, 4000u, 100000u}) {
    Case c = base("sizes/head-from-last-count", 400, 2);
    c.hist.slab_runs = 1u << 18;
    c.hist.last_max_count = last;
    run(c);
  }
  // ---- directed
  for (int w : {2, 3, 5, 8}) {
    Case c = base("directed/no-matrix", 400, w);
    c.sw.shard_epilogue = on(1);
    run(c);
    c.name = "directed/matrix-of-another-world";
    c.hist = after_one_job(w + 1, 65536, 300);
    run(c);
    c.name = "directed/ragged";
    c.hist = after_one_job(w, 65536, 300);
    run(c);
    c.name = "directed/ragged-large";
    c.hist = after_one_job(w, 1u << 20, 70000, 997);
    c.matrix = ragged_matrix(w, 997);
    run(c);
    c.name = "directed/unsupported";
    c.hist.dir_unsupported = true;
    run(c);
  }
  for (int cap : {1, 4, 64, 100000}) {
    Case c = base("directed/forced-cap", 28, 2);
    c.sw.device_epilogue = on(1);
    c.sw.shard_epilogue = on(1);
    c.sw.test_directed_cap = on(cap);
    run(c);  // no matrix: nothing to force yet
    c.hist = after_one_job(2, 4096, 200);
    run(c);  // consumed once: the repeat has the matrix's sizes
    c.hist.dir_cap_forced = true;
    run(c);  // not twice
  }
  for (uint32_t each : {80000000u, 79000000u}) {  // two blocks of 90 000 064 runs are 4.32 GB, of 88 875 064 4.27 GB; 4 GiB = 4.29 GB
    Case c = base("directed/beyond-4-gib", 400, 2);
    c.sw.shard_epilogue = on(1);
    c.hist.slab_runs = 0xf0000000u;
    c.hist.last_max_count = 1000;
    c.hist.dir_counts.assign(4, each);
    c.hist.dir_world = 2;
    run(c);
  }
  // ---- verdict
  for (int w : {1, 2, 3}) {
    for (uint32_t most : {4096u, 4097u, 1u << 16, (1u << 16) + 1}) {  // at head_runs, one beyond, at slab_runs, one beyond
      Case c = base("verdict/largest-count", 28, w);
      c.hist.slab_runs = 1u << 16;
      c.slab.assign((size_t)w, 7);
      c.slab.back() = most;
      run(c);
      if (w == 1) continue;
      c.name = "verdict/largest-count-counted";  // a job that travelled as heads but counted: its matrix is taken, unless
      c.sw.device_epilogue = on(1);              // the head or the slab overflowed
      c.sw.shard_epilogue = on(1);
      run(c);
      c.name = "verdict/largest-count-directed";
      c.hist = after_one_job(w, 1u << 16, 3640);  // (head 4 096 + 64)
      c.slab.back() = most;
      run(c);
    }
  }
  for (int w : {2, 3, 5, 8})
    for (uint32_t over : {0u, 1u}) {  // a block at its cap and one beyond
      Case c = base("verdict/block", 400, w);
      c.sw.shard_epilogue = on(1);
      c.hist = after_one_job(w, 65536, 300);
      c.matrix = ragged_matrix(w);
      for (uint32_t &x : c.matrix) x = with_head_margin(x);
      c.matrix.back() += over;
      run(c);
    }
  {
    Case c = base("verdict/slab-overflow-clears-the-matrix", 400, 3);
    c.sw.shard_epilogue = on(1);
    c.hist = after_one_job(3, 2048, 300);
    c.slab = {100, 5000, 20};
    run(c);
    c.name = "verdict/form-changes-at-the-repeat";  // the last job's count made this one a device job; its own does not
    c = base(c.name, 28, 2);
    c.hist.slab_runs = 1u << 16;
    c.hist.last_max_count = kDeviceEpilogueRuns;
    c.sw.shard_epilogue = on(1);
    c.hist.dir_counts = ragged_matrix(2);
    c.hist.dir_world = 2;
    c.matrix = ragged_matrix(2, 2);
    c.slab = {700, 650};
    run(c);
  }
  // ---- job_end's own decision: does every rank enter the gather of result blocks
  for (int w : {1, 2, 3})
    for (size_t total : {(size_t)(1u << 17) - 1, (size_t)1u << 17})
      for (int sw : {-1, 0, 1})
        for (int device : {0, 1}) {
          Case c = base("end/sharded", 28, w);
          c.sw.device_epilogue = on(device);
          c.sw.test_epilogue_fail_rank = on(1);  // (the device form fails on rank 1 alone: shape_fixed, `sharded` stands)
          if (sw >= 0) c.sw.shard_epilogue = on(sw);
          const std::vector<JobPlan> plans = plans_of(c, c.hist, 0);
          const bool first = sharded_at_end(plans[0], c.sw.shard_epilogue, total);
          for (const JobPlan &p : plans) {
            const bool sharded = sharded_at_end(p, c.sw.shard_epilogue, total);
            const bool was = p.shape_fixed ? p.sharded : (w > 1 && before::shard_epilogue(c.sw.shard_epilogue, total));
            CHECK(sharded == first, "rank %d enters another collective than rank 0", p.shape.rank);
            CHECK(sharded == was, "rank %d: sharded %d, %d before", p.shape.rank, sharded, was);
            CHECK(!sharded || w > 1, "rank %d: one rank gathers nothing", p.shape.rank);
          }
          std::printf("end/sharded: W=%d runs=%zu switch=%d device=%d fixed=%d | sharded=%d\n", w, total, sw, device, plans[0].shape_fixed, first);
        }
  if (g_failed) {
    std::printf("%d invariants failed\n", g_failed);
    return 1;
  }
  std::printf("job plans ok\n");
  return 0;
}
