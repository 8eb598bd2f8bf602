// scan_collect_kernel / group_collect_kernel: PERCENTILE and DISTINCTCOUNT over raw (no-dictionary) INT / LONG / FLOAT / DOUBLE columns as
// compacted lists of the matching docs' values.
//
// What it replaces: PercentileAggregationFunction.aggregate (every matching doc's value appended to a DoubleArrayList) and
// DistinctCountAggregationFunction.aggregate on a column without a dictionary (every value added to an Int / Long / Float / DoubleOpenHashSet),
// and their aggregateGroupBySV forms (one list / set per group).  Without a dictionary there is no dictId to count or to set a bit for
// (pg_scan_counts.h, pg_scan_distinct.h): the kernel writes the 64-bit ORDER IMAGE (pg_order_image.h) of every matching doc's value into a
// list, the engine sorts the list on the query's stream (rocPRIM radix sort) and finds its runs (collect_run_heads_kernel /
// collect_run_compact_kernel).  The sorted (value, count) runs are the percentile's list; the run values alone are the distinct set.
//
// The body is scan_counts_body's (pg_scan_counts.h): the lane-private filter over 2048-doc tiles, a lane holding the match mask m of its 32
// consecutive docs.  Per tile with a match:
//   reserve   popcount(m) goes through a wave-level exclusive prefix sum; lane 0 adds the wave's total to the query's cursor with ONE returning
//             device-scope atomic and the base is broadcast: the wave owns slots [base, base + total), lane l the popcount(m_l) slots from
//             base + prefix_l on, its docs in doc order.  A wave whose base + total would pass the capacity sets kCollectOverflow and writes
//             nothing (the host answers PG_ERR_INTERNAL): no store leaves the allocation whatever the cursor says.
//   write     for every collected column (up to kMaxAggCols; all of them share the slot index) the lane reads its 32 values as stored -- big-
//             endian, sixteen bytes per load, eight-doc pieces without a match skipped -- and stores the images of the matching ones.  Under GROUP
//             BY the docs' raw group ids (distinct_rows16) go to out_rows at the same slots.
// Which wave gets which base differs from run to run: slot order is not deterministic, the sort removes that.
//
// Workgroups of 256 threads like the HBM tiers of the siblings: nothing is shared in LDS but the filter's staged sets and the reduction
// records, and the occupancy is the register file's (waves_scan_collect / waves_group_collect; profiles/kernel_resource_usage.tsv).
//
// Count and filter entries travel in the workgroups' records exactly as scan_counts_body's do (publish_block_partial).
#pragma once
#include "pg_kernels.h"
#include "pg_group_rows.h"
#include "pg_order_image.h"

namespace pg {

// The exclusive prefix sum of v over the wave's 64 lanes (every lane active); total: the wave's sum.
__device__ __forceinline__ uint32_t wave_exclusive_sum_u32(uint32_t v, int lane, uint32_t& total) {
  uint32_t inclusive = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t below = (uint32_t)__shfl_up((int)inclusive, d);
    if (lane >= d) inclusive += below;
  }
  total = (uint32_t)__shfl((int)inclusive, 63);
  return inclusive - v;
}

// The lane's 32 docs of one raw column: the images of the matching ones to out[0 .. popcount(m)), in doc order.
__device__ __forceinline__ void collect_raw64(const uint8_t* __restrict__ fwd, int vkind, long long tile, int lane, uint32_t m, unsigned long long* __restrict__ out) {
  const uint4* src = reinterpret_cast<const uint4*>(fwd + (tile * 2048 + (long long)lane * 32) * 8);
  uint32_t k = 0u;
#pragma unroll 1
  for (int c = 0; c < 4; ++c) {
    const uint32_t mc = (m >> (c * 8)) & 0xFFu;
    if (mc == 0u) continue;
    uint4 w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = src[c * 4 + i];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned long long v0 = ((unsigned long long)__builtin_bswap32(w[i].x) << 32) | (unsigned long long)__builtin_bswap32(w[i].y);
      const unsigned long long v1 = ((unsigned long long)__builtin_bswap32(w[i].z) << 32) | (unsigned long long)__builtin_bswap32(w[i].w);
      if ((mc >> (2 * i)) & 1u) out[k++] = order_image_of_host64(vkind, v0);
      if ((mc >> (2 * i + 1)) & 1u) out[k++] = order_image_of_host64(vkind, v1);
    }
  }
}
__device__ __forceinline__ void collect_raw32(const uint8_t* __restrict__ fwd, int vkind, long long tile, int lane, uint32_t m, unsigned long long* __restrict__ out) {
  const uint4* src = reinterpret_cast<const uint4*>(fwd + (tile * 2048 + (long long)lane * 32) * 4);
  uint32_t k = 0u;
#pragma unroll 1
  for (int c = 0; c < 4; ++c) {
    const uint32_t mc = (m >> (c * 8)) & 0xFFu;
    if (mc == 0u) continue;
    const uint4 w0 = src[c * 2], w1 = src[c * 2 + 1];
    const uint32_t dw[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if ((mc >> j) & 1u) out[k++] = order_image_of_host32(vkind, __builtin_bswap32(dw[j]));
  }
}

template <bool kGroup>
__device__ __forceinline__ void scan_collect_body(const CollectParams& cp, uint32_t* lds) {
  const DistinctParams& dp = cp.d;
  const ScanParams& p = dp.scan;
  const int lane = threadIdx.x & 63;
  const int wave_in_block = threadIdx.x >> 6;
  const int waves_per_block = blockDim.x >> 6;
  const long long total_waves = (long long)gridDim.x * waves_per_block;
  const long long num_tiles = ((long long)p.num_docs + 2047) / 2048;
  // the filter's dictId sets (set_leaves_in_lds = 1 + the area's byte offset, as scan_hist_body)
  uint32_t* set_lds = nullptr;
  if (p.set_leaves_in_lds > 1) { set_lds = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(lds) + (p.set_leaves_in_lds - 1)); stage_filter_sets(p, set_lds); }
  __syncthreads();

  unsigned long long count = 0;
  uint32_t entries = 0u;
  const bool listed = p.tile_list != nullptr;              // index-driven filters: only the tiles index_and_kernel listed hold a match
  const long long tile_limit = listed ? (long long)*p.tile_count : num_tiles;
  for (long long tile_it = (long long)blockIdx.x * waves_per_block + wave_in_block; tile_it < tile_limit; tile_it += total_waves) {
    const long long tile = listed ? (long long)p.tile_list[tile_it] : tile_it;
    uint32_t m = eval_filter_private(p, tile, lane, entries, nullptr, set_lds);
    const long long rem = (long long)p.num_docs - (tile * 2048 + lane * 32);
    m &= rem >= 32 ? 0xFFFFFFFFu : (rem <= 0 ? 0u : ((1u << (int)rem) - 1u));
    const uint32_t mine = (uint32_t)__builtin_popcount(m);
    count += mine;
    if (__builtin_amdgcn_ballot_w64(m != 0u) == 0ull) continue;
    // the wave's slots: one returning atomic per wave and tile
    uint32_t total;
    const uint32_t prefix = wave_exclusive_sum_u32(mine, lane, total);
    unsigned long long base = 0ull;
    if (lane == 0) base = __hip_atomic_fetch_add(cp.cursor, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) | (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
    if (base + (unsigned long long)total > cp.capacity) {      // (wave-uniform)
      if (lane == 0) __hip_atomic_fetch_or(cp.flags, kCollectOverflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    // (a lane without a match loads nothing: see scan_private_kernel)
    if (p.lane_skip == 0 || m != 0u) {
      const unsigned long long at = base + (unsigned long long)prefix;
      if constexpr (kGroup) {
        uint32_t rows0[16], rows1[16];
        distinct_rows16<0>(dp, tile, lane, rows0);
        distinct_rows16<1>(dp, tile, lane, rows1);
        uint32_t* const out = cp.out_rows + at;
        uint32_t k = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) if ((m >> j) & 1u) out[k++] = rows0[j];
#pragma unroll
        for (int j = 0; j < 16; ++j) if ((m >> (16 + j)) & 1u) out[k++] = rows1[j];
      }
#pragma unroll
      for (int c = 0; c < kMaxAggCols; ++c) {
        if (c >= dp.num_cols) break;
        const int vkind = cp.vkind[c];
        if (vkind == kValI64 || vkind == kValF64) collect_raw64(cp.fwd[c], vkind, tile, lane, m, cp.out_images[c] + at);
        else collect_raw32(cp.fwd[c], vkind, tile, lane, m, cp.out_images[c] + at);
      }
    }
  }

  flush_filter_entries(p, entries);
  BlockPartial mine;
  partial_identity(mine);
  mine.count = (unsigned long long)wave_sum_i64((long long)count);
  mine.entries = (unsigned long long)wave_sum_i64((long long)entries);
  __syncthreads();       // every thread is done with the staged sets: the start of LDS becomes the reduction scratch
  BlockPartial* red = reinterpret_cast<BlockPartial*>(lds);
  if (lane == 0) red[wave_in_block] = mine;
  __syncthreads();
  publish_block_partial(p, red, waves_per_block, reinterpret_cast<uint32_t*>(red + waves_per_block), blockIdx.x, gridDim.x);      // (the engine sizes the LDS for it)
}

__global__ __launch_bounds__(kDistinctBlockThreads) void scan_collect_kernel(const CollectParams cp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t collect_lds[];
  scan_collect_body<false>(cp, collect_lds);
}

__global__ __launch_bounds__(kDistinctBlockThreads) void group_collect_kernel(const CollectParams cp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t collect_lds[];
  scan_collect_body<true>(cp, collect_lds);
}

// ---- the runs of a sorted list: flag the run heads, (rocPRIM inclusive scan of the flags,) compact ----
// rows: the list's raw group ids, sorted in front of the images (GROUP BY), or nullptr -- a run ends where the row or the image changes.
__device__ __forceinline__ bool collect_is_head(const unsigned long long* __restrict__ images, const uint32_t* __restrict__ rows, unsigned long long i) {
  return i == 0ull || images[i] != images[i - 1] || (rows != nullptr && rows[i] != rows[i - 1]);
}
__global__ __launch_bounds__(256) void collect_run_heads_kernel(const unsigned long long* __restrict__ images, const uint32_t* __restrict__ rows, unsigned long long n, uint32_t* __restrict__ heads) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x)
    heads[i] = collect_is_head(images, rows, i) ? 1u : 0u;
}
// position[i]: the inclusive scan of heads.  Run j = position - 1 of a head: its image, its first index, (GROUP BY) its row; *num_runs = position[n - 1].
// Every out_* array has room for n runs and is none of the inputs.
__global__ __launch_bounds__(256) void collect_run_compact_kernel(const unsigned long long* __restrict__ images, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ position,
                                                                  unsigned long long n, unsigned long long* __restrict__ out_images, uint32_t* __restrict__ out_first,
                                                                  uint32_t* __restrict__ out_rows, uint32_t* __restrict__ num_runs) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    const uint32_t at = position[i];
    if (i == n - 1) *num_runs = at;
    if (!collect_is_head(images, rows, i)) continue;
    const uint32_t j = at - 1u;      // (at >= 1: doc 0 is a head) j < n
    out_images[j] = images[i];
    out_first[j] = (uint32_t)i;
    if (rows != nullptr) out_rows[j] = rows[i];
  }
}

}  // namespace pg
