// Contiguous block plan of everything that is split across ranks (videos, pairs, hashes): plain C++, no HIP.
#pragma once

#include <algorithm>
#include <cstddef>

namespace needle {

// `units` split into `world` blocks of ceil(units / world); rank's [first, first + count).
inline size_t shard_block(size_t units, int world) { return world > 0 ? (units + (size_t)world - 1) / (size_t)world : units; }
inline void shard_range(size_t units, int world, int rank, size_t *first, size_t *count) {
  const size_t b = shard_block(units, world);
  const size_t f = std::min(units, (size_t)rank * b);
  *first = f;
  *count = std::min(b, units - f);
}

}  // namespace needle
