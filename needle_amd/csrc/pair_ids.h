// The two pair numberings and the way from one to the other, for the host and the device alike (tests/cpp/pair_ids_check.cpp
// runs these very functions on the CPU).  Every intermediate is 64-bit: V (V - 1) / 2 x regions may come close to 2^32.
//   i-major (the comparator's, NeedleHipRun.problem of a cross-matcher over V videos): pair (a, b), a < b, is
//     a (2 V - a - 1) / 2 + (b - a - 1); it depends on V.
//   column-major (the index store's): p(a, b) = b (b - 1) / 2 + a; it does not, so an append adds ids at the end.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEEDLE_HOST_DEVICE __host__ __device__
#else
#define NEEDLE_HOST_DEVICE
#endif

namespace needle {

// first i-major pair of row a: the rows before it hold (V - 1) + (V - 2) + ... + (V - a) pairs
NEEDLE_HOST_DEVICE inline uint64_t row_major_start(uint64_t a, uint64_t V) { return a * (2 * V - a - 1) / 2; }
NEEDLE_HOST_DEVICE inline uint64_t row_major_pair(uint64_t a, uint64_t b, uint64_t V) { return row_major_start(a, V) + (b - a - 1); }
NEEDLE_HOST_DEVICE inline uint64_t column_major_pair(uint64_t a, uint64_t b) { return b * (b - 1) / 2 + a; }

// (a, b) of i-major pair `pair` over V videos; false where there is no such pair.  The last row that starts at or before
// `pair`, by bisection: exact, no floating point.
NEEDLE_HOST_DEVICE inline bool row_major_pair_at(uint64_t pair, uint64_t V, uint32_t *a, uint32_t *b) {
  if (V < 2 || pair >= V * (V - 1) / 2) return false;
  uint64_t lo = 0, hi = V - 2;
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) / 2;
    if (row_major_start(mid, V) <= pair) lo = mid;
    else hi = mid - 1;
  }
  *a = (uint32_t)lo;
  *b = (uint32_t)(lo + 1 + (pair - row_major_start(lo, V)));
  return true;
}

// problem = i-major pair * regions + region -> (a, b, region)
NEEDLE_HOST_DEVICE inline bool decode_problem(uint32_t problem, uint32_t regions, uint64_t V, uint32_t *a, uint32_t *b, uint32_t *r) {
  if (regions == 0) return false;
  *r = problem % regions;
  return row_major_pair_at(problem / regions, V, a, b);
}

// The tag of (a, b, region) in an append onto n0 videos (b >= n0): the store's bucket less the append's first one, p(0, n0).
NEEDLE_HOST_DEVICE inline uint64_t append_tag(uint64_t a, uint64_t b, uint64_t r, uint64_t n0, uint64_t regions) {
  const uint64_t first = n0 ? column_major_pair(0, n0) : 0;
  return (column_major_pair(a, b) - first) * regions + r;
}

}  // namespace needle
