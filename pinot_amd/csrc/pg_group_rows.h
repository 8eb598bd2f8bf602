// distinct_rows16: the raw group id of every doc of a lane's chunk, for the kernels that keep one row per raw group id in HBM
// (group_distinct_kernel of pg_scan_distinct.h, group_counts_kernel of pg_scan_counts.h).
#pragma once
#include "pg_kernels.h"

namespace pg {

constexpr int kDistinctBlockThreads = 256;      // the HBM tiers of both families; their LDS tiers share one bitset / counter vector among kHistBlockThreads

// The raw group ids of sixteen docs: sum over the key columns of dictId * mult (group_private_kernel's key arithmetic; the key space is
// an int, so 32-bit arithmetic does not wrap).
template <int H>
__device__ __forceinline__ void distinct_rows16(const DistinctParams& dp, long long tile, int lane, uint32_t (&rows)[16]) {
#pragma unroll
  for (int j = 0; j < 16; ++j) rows[j] = 0u;
#pragma unroll
  for (int k = 0; k < kMaxDistinctKeys; ++k) {
    if (k >= dp.num_keys) break;
    const DistinctKey& key = dp.keys[k];
    const uint32_t* words = reinterpret_cast<const uint32_t*>(key.fwd + tile * (256ll * key.bits)) + lane * key.bits;
    uint32_t v[16];
    decode16_private_dispatch<H>(key.bits, words, v);
#pragma unroll
    for (int j = 0; j < 16; ++j) rows[j] += v[j] * key.mult;
  }
}

}  // namespace pg
