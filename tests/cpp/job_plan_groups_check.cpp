// Host-side check of needle_amd/csrc/job_plan.h for a library with groups of videos: JobShape::pairs, the job's pair count
// where it is not all pairs of the n videos.  For worlds 1, 2, 3, 5 and 8 and grouped pair counts 0, 1, 6, 16 383, 16 384
// and 65 536 (with 1 and 2 comparator regions, under every history and switch listed below):
//   - the ranks' pair ranges cover [0, P) exactly once, in rank order (a rank with an empty range is allowed);
//   - every rank derives the same form, sizes and caps from the same history, through plan -> judge -> plan until done;
//   - the form follows the pair count, not the videos: the device epilogue from P x regions >= 16 384, sharding from
//     65 536, and never without a pair;
//   - a shape whose pair count equals job_pairs(n) gives a plan equal to the plain shape's in every field.
// Prints "job plan groups ok" and returns 0, or one line per broken invariant.
#include <cstdio>
#include <string>
#include <vector>

#include "../../needle_amd/csrc/job_plan.h"

using namespace needle;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)               \
  do {                                 \
    if (!(cond)) {                     \
      std::printf("INVARIANT ");       \
      std::printf(__VA_ARGS__);        \
      std::printf(" (%s)\n", #cond);   \
      g_failed++;                      \
    }                                  \
  } while (0)

bool same_directed(const DirectedPlan &a, const DirectedPlan &b) {
  return a.wanted == b.wanted && a.sized == b.sized && a.refused == b.refused && a.cap_consumed == b.cap_consumed && a.cap == b.cap &&
         a.send_capacity == b.send_capacity && a.send_off == b.send_off && a.send_bytes == b.send_bytes && a.recv_off == b.recv_off &&
         a.recv_bytes == b.recv_bytes && a.send_total == b.send_total && a.recv_total == b.recv_total && a.max_block_bytes == b.max_block_bytes;
}
bool same_segments(const SegmentLayout &a, const SegmentLayout &b) {
  return a.kind == b.kind && a.capacity == b.capacity && a.capacities == b.capacities && a.max_runs == b.max_runs;
}
// every field of the plan but the shape's own `pairs`
bool same_plan(const JobPlan &a, const JobPlan &b) {
  return a.shape.n == b.shape.n && a.shape.arena_regions == b.shape.arena_regions && a.shape.comparator_regions == b.shape.comparator_regions &&
         a.shape.world == b.shape.world && a.shape.rank == b.shape.rank && a.pair_first == b.pair_first && a.pair_count == b.pair_count &&
         a.video_first == b.video_first && a.video_count == b.video_count && a.device_epilogue == b.device_epilogue && a.sharded == b.sharded &&
         a.shape_fixed == b.shape_fixed && a.inject_epilogue_failure == b.inject_epilogue_failure && a.slab_runs == b.slab_runs &&
         a.head_runs == b.head_runs && a.pinned_bytes == b.pinned_bytes && same_directed(a.directed, b.directed) &&
         same_segments(a.segments, b.segments);
}
// what must not depend on the rank
bool same_everywhere(const JobPlan &a, const JobPlan &b) {
  return a.device_epilogue == b.device_epilogue && a.sharded == b.sharded && a.shape_fixed == b.shape_fixed && a.slab_runs == b.slab_runs &&
         a.head_runs == b.head_runs && a.pinned_bytes == b.pinned_bytes && a.directed.wanted == b.directed.wanted &&
         a.directed.sized == b.directed.sized && a.directed.refused == b.directed.refused && a.directed.cap == b.directed.cap &&
         a.directed.max_block_bytes == b.directed.max_block_bytes && a.segments.kind == b.segments.kind;
}

JobHook on(int v) { return JobHook{true, v}; }

struct Setting {
  const char *name;
  JobSwitches sw;
  uint32_t last_max_count;  // of the history the first job starts from
};

// One library of `n` videos with `pairs` grouped pairs on `world` ranks: three jobs in a row, every rank planning each
// attempt from the same history and judging the same counts (every rank finds `found` runs, and directs a share to each).
void run_library(const Setting &st, size_t n, uint64_t pairs, size_t regions, int world, uint32_t found) {
  const size_t W = (size_t)world;
  std::vector<JobHistory> hist(W);
  for (JobHistory &h : hist) h.last_max_count = st.last_max_count;
  for (int job = 0; job < 3; job++) {
    uint32_t keep_head = 0;
    for (int attempt = 0; attempt < 8; attempt++) {
      std::vector<JobPlan> plans;
      for (int r = 0; r < world; r++) {
        JobShape sh;
        sh.n = n;
        sh.arena_regions = regions;
        sh.comparator_regions = regions;
        sh.world = world;
        sh.rank = r;
        sh.pairs = pairs;
        plans.push_back(plan_job(sh, st.sw, hist[(size_t)r], keep_head));
      }
      // the ranges cover [0, P) exactly once, in rank order
      size_t at = 0;
      for (size_t r = 0; r < W; r++) {
        const JobPlan &p = plans[r];
        CHECK(p.pair_first == at || p.pair_count == 0, "%s P=%llu world %d rank %zu: range starts at %zu, not %zu", st.name,
              (unsigned long long)pairs, world, r, p.pair_first, at);
        CHECK(p.pair_first + p.pair_count <= pairs, "%s P=%llu world %d rank %zu: range beyond the pairs", st.name, (unsigned long long)pairs, world, r);
        at += p.pair_count;
        CHECK(same_everywhere(p, plans[0]), "%s P=%llu world %d rank %zu plans another job than rank 0", st.name, (unsigned long long)pairs, world, r);
        // the form follows the pair count
        CHECK(pairs > 0 || !p.device_epilogue, "%s world %d: a job without a pair takes the host form", st.name, world);
        if (!st.sw.device_epilogue.set && st.last_max_count == 0 && job == 0 && attempt == 0)
          CHECK(p.device_epilogue == (pairs * regions >= 16384), "%s P=%llu x %zu world %d: device epilogue %d", st.name,
                (unsigned long long)pairs, regions, world, (int)p.device_epilogue);
        if (p.device_epilogue && !st.sw.shard_epilogue.set && !st.sw.shard_epilogue_pairs.set)
          CHECK(p.sharded == (world > 1 && pairs * regions >= 65536), "%s P=%llu x %zu world %d: sharded %d", st.name, (unsigned long long)pairs,
                regions, world, (int)p.sharded);
        if (attempt == 0 && job == 0 && !st.sw.slab_runs.set)
          CHECK(p.slab_runs == round_up4(std::max<uint64_t>(1024, 4 * (uint64_t)shard_block((size_t)pairs, world) * regions)),
                "%s P=%llu world %d: the first slab is sized by the job's pairs (%u)", st.name, (unsigned long long)pairs, world, p.slab_runs);
        CHECK(p.head_runs <= p.slab_runs && p.head_runs % 4 == 0 && p.slab_runs % 4 == 0, "%s: head %u slab %u", st.name, p.head_runs, p.slab_runs);
      }
      CHECK(at == pairs, "%s world %d: the ranges hold %zu pairs of %llu", st.name, world, at, (unsigned long long)pairs);
      // the counts every rank sees: `found` runs per rank that has pairs, spread evenly over the destinations
      JobCounts c;
      c.directed = plans[0].directed.wanted && plans[0].directed.sized;
      for (size_t r = 0; r < W; r++) c.slab.push_back(plans[r].pair_count ? found : 0u);
      if (plans[0].directed.wanted)
        for (size_t r = 0; r < W; r++)
          for (size_t q = 0; q < W; q++) c.directed_to.push_back(c.slab[r] / (uint32_t)W + 1);
      JobNext next = JobNext::Done;
      for (size_t r = 0; r < W; r++) {
        JobHistory before = hist[r];
        before.slab_runs = plans[r].slab_runs;  // (a first slab sticks: library.cpp job_plan_stage)
        if (plans[r].directed.cap_consumed) before.dir_cap_forced = true;
        const JobVerdict v = judge(plans[r], c, before);
        if (r == 0) next = v.next;
        CHECK(v.next == next, "%s world %d rank %zu draws another verdict than rank 0", st.name, world, r);
        hist[r] = v.history;
        keep_head = v.keep_head;
      }
      if (next == JobNext::Done) break;
      CHECK(attempt < 7, "%s P=%llu world %d: the repeat loop does not end", st.name, (unsigned long long)pairs, world);
    }
  }
}

}  // namespace

int main() {
  std::vector<Setting> settings;
  settings.push_back({"defaults", JobSwitches(), 0});
  settings.push_back({"last-count", JobSwitches(), 70000});
  {
    JobSwitches sw;
    sw.device_epilogue = on(1);
    sw.shard_epilogue = on(1);
    settings.push_back({"device-sharded", sw, 0});
    sw.test_directed_cap = on(4);
    settings.push_back({"device-sharded-cap", sw, 0});
    sw = JobSwitches();
    sw.device_epilogue = on(0);
    settings.push_back({"host", sw, 0});
    sw = JobSwitches();
    sw.slab_runs = on(4);
    settings.push_back({"slab-4", sw, 0});
    sw.device_epilogue = on(1);
    sw.shard_epilogue = on(1);
    settings.push_back({"slab-4-device-sharded", sw, 0});
  }
  const int worlds[] = {1, 2, 3, 5, 8};
  const uint64_t pair_counts[] = {0, 1, 6, 16383, 16384, 65536};
  for (const Setting &st : settings)
    for (int world : worlds)
      for (uint64_t pairs : pair_counts)
        for (size_t regions = 1; regions <= 2; regions++)
          for (uint32_t found : {0u, 40u, 5000u}) run_library(st, 2000, pairs, regions, world, found);

  // a shape whose pair count equals job_pairs(n): the plain shape's plan, in every field
  for (const Setting &st : settings)
    for (int world : worlds)
      for (size_t n : {1, 2, 3, 8, 182, 363, 2000})
        for (size_t regions = 1; regions <= 2; regions++)
          for (int rank = 0; rank < world; rank++) {
            JobHistory h;
            h.last_max_count = st.last_max_count;
            for (int with_matrix = 0; with_matrix < 2; with_matrix++) {
              if (with_matrix) {
                h.dir_world = world;
                h.dir_counts.assign((size_t)world * (size_t)world, 33u);
              }
              JobShape plain;
              plain.n = n;
              plain.arena_regions = 2;
              plain.comparator_regions = regions;
              plain.world = world;
              plain.rank = rank;
              JobShape grouped = plain;
              grouped.pairs = job_pairs(n);
              CHECK(plain.pairs == JobShape::kAllPairs && plain.pair_total() == job_pairs(n), "the default is all pairs");
              CHECK(same_plan(plan_job(plain, st.sw, h), plan_job(grouped, st.sw, h)), "%s n=%zu world %d rank %d: one group is not the plain plan",
                    st.name, n, world, rank);
            }
          }
  if (g_failed) {
    std::printf("%d invariants broken\n", g_failed);
    return 1;
  }
  std::printf("job plan groups ok\n");
  return 0;
}
