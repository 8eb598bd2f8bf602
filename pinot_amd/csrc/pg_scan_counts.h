// scan_counts_kernel / group_counts_kernel: PERCENTILE over dictionary columns as dictId count histograms.
//
// What it replaces: PercentileAggregationFunction.aggregate (core/query/aggregation/function/PercentileAggregationFunction.java:77-100:
// every matching doc's value is appended to one DoubleArrayList) and aggregateGroupBySV (one list per group); the lists are concatenated
// and sorted at the broker (extractFinalResult :155-172).  On a dictionary column the list is fully described by HOW MANY matching docs
// carry each dictId -- the dictionary is sorted, so the sorted list is "dictionary[d], counts[d] times, d ascending".  Per doc the work is
// "counter[dictId] += match" behind the filter: scan_distinct_body (pg_scan_distinct.h) with an add where the bitset has an OR, and a
// vector of 32-bit counters where it has a bitset.  The percentile itself never reaches the device: the vector is the intermediate
// result whatever p is.
//
// Two tiers, one body (the parameter block is DistinctParams: DistinctCol.set_bits = the counters, .words = the cardinality):
//   kLds = true   every PERCENTILE column (up to kMaxAggCols) keeps its 32-bit counters in the workgroup's dynamic LDS, side by side
//                 from word 0; one non-returning workgroup-scope add of the match bit per doc -- unconditional, as
//                 hist16_private<..., 32, false> does it: a doc that does not match adds zero.  At the end every workgroup adds its
//                 non-zero counters into the query's zeroed vector in HBM (device-scope atomic, result unused).  A workgroup sees
//                 fewer than 2^31 docs, so a 32-bit counter cannot wrap: none of scan_hist_kernel's guard / checksum tiers.
//                 About 39 000 dictIds over all columns fit (the engine's scan_grid: counters + set area + records <= kLdsBudget).
//                 This tier TRUSTS the forward index, as the LDS tiers of scan_hist_kernel and scan_distinct_kernel do: a dictId at
//                 or above the cardinality (a corrupt segment) indexes past its column's counters, into a neighbouring column's or
//                 the filter's set area of the same workgroup's LDS -- a wrong answer for that query, never a write outside the
//                 workgroup's LDS allocation's hardware bounds.  The HBM tiers, where a stray index would leave the allocation,
//                 keep room for it (the engine's counts_slack_words: 2^bits - cardinality counters behind the last one).
//   kLds = false  one device-scope non-returning atomicAdd per MATCHING doc straight into the zeroed vector in HBM.  Any cardinality;
//                 PINOT_GPU_PERCENTILE_LDS=0 sends every query here.
//   kGroup        (HBM only) the raw group id of each matching doc (distinct_rows16) selects row g of a
//                 [group_id_upper_bound x cardinality] counter matrix per column.
//
// Not built: narrow (8 / 16-bit) LDS counters for 39 k - 155 k dictIds, wave-level pre-aggregation of hot
// dictIds in the HBM tier, compacting the matrix on the device.
//
// Count and filter entries travel in the workgroups' records exactly as scan_hist_body's do (publish_block_partial).
#pragma once
#include "pg_kernels.h"
#include "pg_group_rows.h"

namespace pg {

// Sixteen docs (half H) of the lane's chunk of one PERCENTILE column.  rows: kGroup -- the docs' raw group ids.
template <bool kLds, bool kGroup, int H>
__device__ __forceinline__ void counts16(int b, const uint32_t* __restrict__ lane_words, uint32_t m, uint32_t* counters, int cardinality, const uint32_t (&rows)[16]) {
  uint32_t v[16];
  decode16_private_dispatch<H>(b, lane_words, v);
  if constexpr (kLds) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      __hip_atomic_fetch_add(counters + v[j], __builtin_amdgcn_ubfe(m, 16 * H + j, 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (((m >> (16 * H + j)) & 1u) == 0u) continue;
      uint32_t* const w = counters + (kGroup ? (size_t)rows[j] * (size_t)cardinality : (size_t)0) + v[j];
      __hip_atomic_fetch_add(w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <bool kLds, bool kGroup>
__device__ __forceinline__ void scan_counts_body(const DistinctParams& dp, uint32_t* lds) {
  static_assert(!(kLds && kGroup), "the counter matrix of a group-by lives in HBM");
  const ScanParams& p = dp.scan;
  const int lane = threadIdx.x & 63;
  const int wave_in_block = threadIdx.x >> 6;
  const int waves_per_block = blockDim.x >> 6;
  const long long total_waves = (long long)gridDim.x * waves_per_block;
  const long long num_tiles = ((long long)p.num_docs + 2047) / 2048;
  if constexpr (kLds) for (int w = threadIdx.x; w < dp.lds_words; w += blockDim.x) lds[w] = 0u;
  // the filter's dictId sets behind the counters (set_leaves_in_lds = 1 + the area's byte offset, as scan_hist_body)
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
    count += (unsigned)__builtin_popcount(m);
    if (__builtin_amdgcn_ballot_w64(m != 0u) == 0ull) continue;
    // (a lane without a match loads nothing: see scan_private_kernel)
    if (p.lane_skip == 0 || m != 0u) {
      uint32_t rows0[16], rows1[16];
      if constexpr (kGroup) { distinct_rows16<0>(dp, tile, lane, rows0); distinct_rows16<1>(dp, tile, lane, rows1); }
#pragma unroll
      for (int c = 0; c < kMaxAggCols; ++c) {
        if (c >= dp.num_cols) break;
        const DistinctCol& col = dp.cols[c];
        const uint32_t* words = reinterpret_cast<const uint32_t*>(col.fwd + tile * (256ll * col.bits)) + lane * col.bits;
        uint32_t* const target = kLds ? lds + col.lds_off : col.set_bits;
        counts16<kLds, kGroup, 0>(col.bits, words, m, target, col.words, rows0);
        counts16<kLds, kGroup, 1>(col.bits, words, m, target, col.words, rows1);
      }
    }
  }

  if constexpr (kLds) {
    // the workgroup's counters -> the query's: only the ones that counted a doc
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kMaxAggCols; ++c) {
      if (c >= dp.num_cols) break;
      const DistinctCol& col = dp.cols[c];
      for (int w = threadIdx.x; w < col.words; w += blockDim.x) {
        const uint32_t n = lds[col.lds_off + w];
        if (n != 0u) __hip_atomic_fetch_add(col.set_bits + w, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }

  flush_filter_entries(p, entries);
  BlockPartial mine;
  partial_identity(mine);
  mine.count = (unsigned long long)wave_sum_i64((long long)count);
  mine.entries = (unsigned long long)wave_sum_i64((long long)entries);
  __syncthreads();       // every thread is done with the counters: the start of LDS becomes the reduction scratch
  BlockPartial* red = reinterpret_cast<BlockPartial*>(lds);
  if (lane == 0) red[wave_in_block] = mine;
  __syncthreads();
  publish_block_partial(p, red, waves_per_block, reinterpret_cast<uint32_t*>(red + waves_per_block), blockIdx.x, gridDim.x);      // (the engine sizes the LDS for it)
}

template <bool kLds>
__global__ __launch_bounds__(kLds ? kHistBlockThreads : kDistinctBlockThreads) void scan_counts_kernel(const DistinctParams dp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t counts_lds[];      // the only LDS object: counter addresses need no base add
  scan_counts_body<kLds, false>(dp, counts_lds);
}

__global__ __launch_bounds__(kDistinctBlockThreads) void group_counts_kernel(const DistinctParams dp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t counts_lds[];
  scan_counts_body<false, true>(dp, counts_lds);
}

}  // namespace pg
