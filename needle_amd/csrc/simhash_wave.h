// chromaprint's simhash32 of a slice of hashes by one wave (comparator.rs:149-153): the arithmetic the run-reporting
// kernels share (search.hip simhash_runs_kernel; stream_walk.h simhash_runs, the body of matcher_simhash_kernel and
// crossmatch_simhash_kernel).  How it works, and what it replaced, is told in search.hip above simhash_runs_kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace needle {

struct TransposeLane {  // per-lane constants of the five steps
  uint32_t rot[5], mask[5];
};
__device__ __forceinline__ TransposeLane transpose_lane(uint32_t lane) {
  TransposeLane t;
  uint32_t m = 0x0000FFFFu;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const uint32_t j = 16u >> k;
    const bool hi = (lane & j) != 0u;
    t.rot[k] = hi ? 32u - j : j;          // rotate right: low lanes take the partner's bits from j places up, high lanes from j down
    t.mask[k] = hi ? m << j : m;
    m ^= m << (j >> 1);
  }
  return t;
}
template <int PATTERN>
__device__ __forceinline__ uint32_t swizzle_xor(uint32_t x) {  // lane ^ (PATTERN >> 10) within 32 lanes: LDS crossbar, no memory
  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, PATTERN);
}
// x: one hash per lane -> lane i (of each half of the wave): bit column 31 - i of its half's 32 hashes
__device__ __forceinline__ uint32_t transpose32(uint32_t x, const TransposeLane &t) {
#define NEEDLE_TSTEP(K, J)                                                              \
  {                                                                                     \
    const uint32_t y = swizzle_xor<((J) << 10) | 0x1F>(x);                              \
    const uint32_t r = __builtin_amdgcn_alignbit(y, y, t.rot[K]);                      \
    x = (r & t.mask[K]) | (x & ~t.mask[K]);                                             \
  }
  NEEDLE_TSTEP(0, 16) NEEDLE_TSTEP(1, 8) NEEDLE_TSTEP(2, 4) NEEDLE_TSTEP(3, 2) NEEDLE_TSTEP(4, 1)
#undef NEEDLE_TSTEP
  return x;
}
__device__ __forceinline__ uint32_t wave_simhash32(const uint32_t *__restrict__ slice, uint32_t count, uint32_t lane, const TransposeLane &t) {
  constexpr int kBlocks = 8;                       // 512 hashes per turn
  uint32_t ones = 0;                               // lane i: hashes of its half (so far) with bit 31 - (i & 31) set
  for (uint32_t q0 = 0; q0 < count; q0 += 64 * kBlocks) {
    uint32_t h[kBlocks];
#pragma unroll
    for (int u = 0; u < kBlocks; u++) {
      const uint32_t q = q0 + 64 * u + lane;
      h[u] = q < count ? slice[q] : 0u;            // beyond the slice: no ones
    }
#pragma unroll
    for (int u = 0; u < kBlocks; u++) {
      if (q0 + 64 * u >= count) break;             // (wave-uniform)
      ones += (uint32_t)__popc(transpose32(h[u], t));
    }
  }
  ones += (uint32_t)__shfl_xor((int)ones, 32);     // both halves' hashes
  // bit 31 - i set iff ones > zeros (a tie leaves it clear): lanes 0 .. 31 give the word, bit-reversed
  const unsigned long long set = __builtin_amdgcn_ballot_w64(2u * ones > count);
  return __brev((uint32_t)set);
}

}  // namespace needle
