// needle_amd/csrc/pair_ids.h on the CPU: the very functions index_ingest_runs_kernel runs per run.  A cross-matcher over V
// videos, the first K of them resident, names a run's pair in the comparator's i-major order; the index store wants the
// column-major id less the append's first.  Both against the enumerations themselves, for every V <= 48, every K <= V and
// R in {1, 2}; then the largest V whose problem index still fits 32 bits, where a 32-bit intermediate would wrap.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pair_ids.h"

using namespace needle;

static int fail(const char *what, uint64_t V, uint64_t K, uint64_t R, uint64_t a, uint64_t b) {
  std::printf("FAIL %s: V=%llu K=%llu R=%llu pair (%llu, %llu)\n", what, (unsigned long long)V, (unsigned long long)K, (unsigned long long)R,
              (unsigned long long)a, (unsigned long long)b);
  return 1;
}

int main() {
  for (uint64_t V = 2; V <= 48; V++) {
    // the store's numbering by enumeration: column after column
    std::vector<std::vector<uint64_t>> column(V, std::vector<uint64_t>(V, 0));
    uint64_t next = 0;
    for (uint64_t b = 1; b < V; b++)
      for (uint64_t a = 0; a < b; a++) column[a][b] = next++;
    for (uint64_t R = 1; R <= 2; R++)
      for (uint64_t K = 0; K <= V; K++) {
        const uint64_t first = K * (K ? K - 1 : 0) / 2;  // pairs among the K old videos: the ids below the append's
        uint64_t problem = 0;                            // the comparator's numbering by enumeration: i-major
        std::vector<uint8_t> seen((V * (V - 1) / 2 - first) * R, 0);
        for (uint64_t a = 0; a + 1 < V; a++)
          for (uint64_t b = a + 1; b < V; b++)
            for (uint64_t r = 0; r < R; r++, problem++) {
              if (row_major_pair(a, b, V) * R + r != problem) return fail("row_major_pair", V, K, R, a, b);
              uint32_t da = 0, db = 0, dr = 0;
              if (!decode_problem((uint32_t)problem, (uint32_t)R, V, &da, &db, &dr) || da != a || db != b || dr != r)
                return fail("decode_problem", V, K, R, a, b);
              if (b < K) continue;  // an old pair: no live problem of the matcher
              const uint64_t tag = append_tag(a, b, r, K, R);
              if (tag != (column[a][b] - first) * R + r || tag >= seen.size() || seen[tag]) return fail("append_tag", V, K, R, a, b);
              seen[tag] = 1;
            }
        for (uint8_t s : seen)
          if (!s) return fail("append_tag does not cover the append's buckets", V, K, R, 0, 0);
        uint32_t da, db, dr;
        if (decode_problem((uint32_t)problem, (uint32_t)R, V, &da, &db, &dr)) return fail("decode_problem beyond the last pair", V, K, R, 0, 0);
      }
  }
  uint32_t da, db, dr;
  if (decode_problem(0, 1, 1, &da, &db, &dr) || decode_problem(0, 1, 0, &da, &db, &dr) || decode_problem(0, 0, 5, &da, &db, &dr)) {
    std::printf("FAIL: a pair where there is none\n");
    return 1;
  }
  // The largest V with V (V - 1) / 2 x R < 2^32: at V = 92 682 a (2 V - a - 1) passes 2^32 from a = 27 146 on, b (b - 1) from b = 65 537 on.
  // Every row's first two and last pairs and one in the middle, against a running sum of the row lengths.
  const uint64_t largest[2] = {92682, 65536};
  for (uint64_t R = 1; R <= 2; R++) {
    const uint64_t V = largest[R - 1];
    if (V * (V - 1) / 2 * R >= (1ull << 32) || (V + 1) * V / 2 * R < (1ull << 32)) return fail("not the largest V", V, 0, R, 0, 0);
    uint64_t start = 0;
    for (uint64_t a = 0; a + 1 < V; a++) {
      const uint64_t picks[4] = {a + 1, a + 2 < V ? a + 2 : a + 1, (a + 1 + V - 1) / 2, V - 1};
      for (uint64_t b : picks)
        for (uint64_t r = 0; r < R; r++) {
          const uint64_t problem = (start + (b - a - 1)) * R + r;
          if (problem >> 32) return fail("the problem does not fit", V, 0, R, a, b);
          if (row_major_pair(a, b, V) * R + r != problem) return fail("row_major_pair (large)", V, 0, R, a, b);
          if (!decode_problem((uint32_t)problem, (uint32_t)R, V, &da, &db, &dr) || da != a || db != b || dr != r)
            return fail("decode_problem (large)", V, 0, R, a, b);
          for (uint64_t K : {(uint64_t)0, (uint64_t)1, b / 2, b}) {
            // column b starts after 1 + 2 + ... + (b - 1) pairs; the even factor halved first, so no product here passes 2^33
            const uint64_t col = (b % 2 ? b * ((b - 1) / 2) : (b / 2) * (b - 1)), old = (K % 2 ? K * ((K - 1) / 2) : (K / 2) * (K ? K - 1 : 0));
            if (append_tag(a, b, r, K, R) != (col + a - old) * R + r) return fail("append_tag (large)", V, K, R, a, b);
          }
        }
      start += V - 1 - a;
    }
    if (start != V * (V - 1) / 2) return fail("row lengths", V, 0, R, 0, 0);
    if (decode_problem((uint32_t)(start * R - 1), (uint32_t)R, V, &da, &db, &dr) == false || da != V - 2 || db != V - 1 || dr != R - 1)
      return fail("the last problem", V, 0, R, V - 2, V - 1);
  }
  std::printf("pair ids ok\n");
  return 0;
}
