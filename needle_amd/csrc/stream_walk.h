// The device code the two streaming comparators share (matcher.hip, crossmatch.hip): one diagonal walk, the wave-aggregated
// run push, and the bodies of their land and simhash kernels.
//
// The walk.  Two sequences X and Y, items numbered from 0; cell (x, y) matches when the two hashes are within `threshold`
// bits, and a run is a stretch of matching cells along a diagonal.  A round gives Y the new items [y0, y1), the strip, at
// most kMaxStrip of them; X holds x1 items by the end of the round.  Every new cell lies on one diagonal, and a diagonal is
// either CARRIED -- it crosses Y's item y0 - 1 at X's item t and starts from frontier entry from[t], the length of the
// matching stretch that ends there -- or it ENTERS through X's item 1 at one of the strip's items 1 .. W - 1 and starts at
// 0.  A side has `side_blocks` workgroups of kCarriedRows carried diagonals, four per thread one after the other, then
// kTopBlocks of kThreads entering ones; those a round does not need leave at once.  A workgroup stages the X items its
// diagonals meet and the strip in LDS; the loop over the strip is uniform for it, so the runs of one step leave a wave
// together (push_runs).  A mismatch after >= min_len matches reports the run that ended one cell before.  Where a diagonal
// stops it hands its length on: in Y's new last item to to_last_y (by X position), in X's last item to to_last_x (by Y
// position).  A round never writes what it reads, so it can be repeated (stream_round.h: the run slab).
//
// The rules, one each, for every user:
//   Item 0 is no cell.  The caller clamps: x1, y0, y1 are at least 1, so no cell test is in the loop, and `from` is
//     nullptr -- all zero -- while either side held fewer than two items before the round: an entry that was never written
//     (or was written for a lane since reset) is never read.  Entry 0 is never read either: its length is 0.
//   A complete X (x_complete: a matcher's source, a cross-matcher's resident row; column direction only).  X gains no items,
//     so a run that reaches its last item cannot grow: it is pushed in that round, where >= min_len, the corner of X's last
//     item and Y's new last item included.  The carried diagonals are entries 1 .. len - 2 (`carried` = len - 1); entry
//     len - 1 is neither written nor read, and nothing goes to to_last_x.  When such a run is handed out is the host's
//     business: the matcher at once, the cross-matcher, as before, when the arriving lane finishes.  No second corner policy.
//   Where X still grows (the cross-matcher's arriving pairs) the corner of X's last item and Y's new last item belongs to
//     the column frontier: to_last_y in the column direction, to_last_x in the row direction.
//   What is open on a frontier (emit_open; the strip is empty then): one loop for every user, ahead of the walk (a branch
//     inside it cost the walk of a few lanes 3 - 5 %): the carried lengths >= min_len are pushed at (t, y0 - 1), nothing written.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "simhash_wave.h"

namespace needle {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxStrip = 512;      // new items of one round per lane
constexpr uint32_t kCarriedRows = 1024;  // carried diagonals per workgroup: four per thread, one after the other
constexpr uint32_t kTopBlocks = (kMaxStrip - 1 + kThreads - 1) / kThreads;  // of entering diagonals, for the widest strip

// The runs a wave wants to report in one step leave together: ballot, ONE returning atomic for all of them, a prefix count
// for the slots (search.hip, round 6); beyond `capacity` they are only counted (the host repeats the round with a larger
// slab).  `make` builds the record of a lane that wants one.  Every lane of the wave comes through here together.
template <typename Run, typename Make>
__device__ __forceinline__ void push_runs(const bool want, Run *__restrict__ runs, const uint32_t capacity, uint32_t *__restrict__ count,
                                          const Make make) {
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(want);
  if (mask == 0ull) return;
  uint32_t base = 0u;
  if ((threadIdx.x & 63u) == 0u) base = atomicAdd(count, (uint32_t)__popcll(mask));
  base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
  const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
  if (want && slot < capacity) runs[slot] = make();
}

// One direction of a round: X is the side the carried diagonals are numbered along, Y the side whose new items are the strip.
template <typename T>
struct WalkSide {
  const uint32_t *xh, *yh;   // the two sequences
  uint32_t x1;               // X's items after the round ...
  uint32_t y0, y1;           // ... and Y's before and after it, each at least 1
  uint32_t carried;          // carried diagonals: entries 0 .. carried - 1 of `from`
  const T *from;             // frontier read, by X position; nullptr: all zero
  T *to_last_y, *to_last_x;  // frontier written where a diagonal stops in Y's new last item (by X position) / in X's (by Y position)
  bool x_complete;           // column direction only: X gains no items, a run that stops in its last item is final
};

// `strip` holds kMaxStrip words of LDS, `rows` kCarriedRows + kMaxStrip; `blk` is the workgroup's number on its side; kCol: X
// is the source (src_end = x), otherwise the transpose; sink(src_end, dst_end, len) is the caller's record.  Whole workgroups only.
template <typename T, bool kCol, typename Run, typename Sink>
__device__ __forceinline__ void stream_walk(uint32_t *__restrict__ strip, uint32_t *__restrict__ rows, const WalkSide<T> &sd, const uint32_t blk,
                                            const uint32_t side_blocks, const bool emit_open, const uint32_t threshold, const uint32_t min_len,
                                            Run *__restrict__ runs, const uint32_t capacity, uint32_t *__restrict__ count, const Sink sink) {
  const uint32_t tid = threadIdx.x;
  const bool carried = blk < side_blocks;
  auto push = [&](const bool want, const uint32_t x, const uint32_t y, const uint32_t len) {
    push_runs(want, runs, capacity, count, [&] { return sink(kCol ? x : y, kCol ? y : x, len); });
  };
  const uint32_t t0 = blk * kCarriedRows;
  if (emit_open) {  // what is open on this side of the frontier (whole waves; min_len >= 1: an entry that is not read reports nothing)
    for (uint32_t part = 0; carried && part < kCarriedRows; part += kThreads) {
      const uint32_t t = t0 + part + tid;
      const uint32_t run = t < sd.carried && t >= 1u && sd.from ? (uint32_t)sd.from[t] : 0u;
      push(run >= min_len, t, sd.y0 - 1u, run);
    }
    return;
  }
  const uint32_t W = sd.y1 - sd.y0;
  if (W == 0u) return;
  // carried: the diagonals that leave frontier entries t0 ..; otherwise those that enter through X's item 1 at the strip's items q0 ..
  const uint32_t q0 = carried ? 0u : (blk - side_blocks) * kThreads + 1u;
  if (carried ? t0 >= sd.carried : q0 >= W) return;  // (the whole workgroup)
  const uint32_t seg0 = carried ? t0 + 1u : 1u;       // first X item staged
  const uint32_t steps = W - q0;                      // the most cells one of the workgroup's diagonals walks
  {
    const uint32_t seg_rows = min(sd.x1 - seg0, (carried ? kCarriedRows : kThreads) - 1u + steps);  // items seg0 .. <= x1 - 1
    const uint32_t *__restrict__ src = sd.xh + seg0;
    for (uint32_t k = tid; k < seg_rows; k += kThreads) rows[k] = src[k];
    for (uint32_t k = tid; k < W; k += kThreads) strip[k] = sd.yh[sd.y0 + k];
  }
  __syncthreads();

  // One diagonal per thread: first new cell (X = i0, Y = y0 + q), `rel` = i0's place in the staged items, `run` = the carried
  // length.  It walks w cells (i0 + c, y0 + q + c).
  auto walk = [&](const bool live, const uint32_t i0, const uint32_t q, const uint32_t rel, uint32_t run) {
    const uint32_t w = live ? min(W - q, sd.x1 - i0) : 0u;
    for (uint32_t c = 0; c < steps; c++) {
      bool ended = false;
      uint32_t len = 0u;
      if (c < w) {
        const bool match = (uint32_t)__popc(rows[rel + c] ^ strip[q + c]) <= threshold;
        ended = !match && run >= min_len;  // the run ended at the previous cell
        len = run;
        run = match ? run + 1u : 0u;
      }
      push(ended, i0 + c - 1u, sd.y0 + q + c - 1u, len);
    }
    // the last cell walked (with no cell: the frontier entry itself, which changes hands)
    const uint32_t x = i0 + w - 1u, y = sd.y0 + q + w - 1u;
    const bool last_y = q + w == W, last_x = x == sd.x1 - 1u;
    const bool final = kCol && sd.x_complete && last_x;
    if (kCol && sd.x_complete) push(live && final && run >= min_len, x, y, run);  // (the whole workgroup or none of it)
    if (!live || final) return;
    if (kCol ? last_y : !last_x) sd.to_last_y[x] = (T)run;
    else sd.to_last_x[y] = (T)run;
  };
  if (carried) {
    for (uint32_t part = 0; part < kCarriedRows; part += kThreads) {
      const uint32_t t = t0 + part + tid;  // leaves frontier entry t (entry 0 is no cell: its length is 0)
      if (t - tid >= sd.carried) break;    // (the whole workgroup)
      const bool live = t < sd.carried;
      const uint32_t run = live && t >= 1u && sd.from ? (uint32_t)sd.from[t] : 0u;
      walk(live, t + 1u, 0u, part + tid, run);
    }
  } else {
    const uint32_t q = q0 + tid;  // enters through X's item 1 at Y's item y0 + q
    walk(q < W, 1u, q, 0u, 0u);
  }
}

// The body of a land kernel: grid (strip / kThreads, lanes of the round's table).  The new chunks go from the round's
// staging buffer (the lane table, then the chunks) to the end of their lanes' histories, and the run counter is cleared.
// A Lane has fed, width and stage_off; history(lane entry) is where the lane's hashes lie.
template <typename Lane, typename History>
__device__ __forceinline__ void land_chunks(const uint32_t *__restrict__ round_buf, uint32_t *__restrict__ count, const History history) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *count = 0u;
  const Lane ln = reinterpret_cast<const Lane *>(round_buf)[blockIdx.y];
  const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
  if (c < ln.width) history(ln)[ln.fed + c] = round_buf[ln.stage_off + c];
}

// The body of a simhash kernel: both simhashes of every run reported, one wave per run.  src(run) and dst(run) are the
// sequences the run's ends count along (wave-uniform); nullptr: that simhash stays 0.
template <typename Run, typename Src, typename Dst>
__device__ __forceinline__ void simhash_runs(Run *__restrict__ runs, const uint32_t capacity, const uint32_t *__restrict__ count, const Src src,
                                             const Dst dst) {
  const uint32_t total = min(*count, capacity);
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  const TransposeLane t = transpose_lane(lane);
  for (uint32_t k = wave; k < total; k += waves) {
    const Run r = runs[k];
    const uint32_t *const s = src(r), *const d = dst(r);
    const uint32_t src_hash = s ? wave_simhash32(s + (r.src_end - r.len), r.len + 1u, lane, t) : 0u;
    const uint32_t dst_hash = d ? wave_simhash32(d + (r.dst_end - r.len), r.len + 1u, lane, t) : 0u;
    if (lane == 0) {
      runs[k].src_match_hash = src_hash;
      runs[k].dst_match_hash = dst_hash;
    }
  }
}

}  // namespace needle
