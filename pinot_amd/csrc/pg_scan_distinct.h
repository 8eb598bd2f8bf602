// scan_distinct_kernel / group_distinct_kernel: DISTINCTCOUNT over dictionary columns as dictId bitsets.
//
// What it replaces: BaseDistinctAggregateAggregationFunction.svAggregate (core/query/aggregation/function/
// BaseDistinctAggregateAggregationFunction.java:144-155: every block's dictIds go into one RoaringBitmap with addN) and
// svAggregateGroupBySV (:306-321: one dictId bitmap per group).  The bitmap turns into a value set once per segment
// (extractAggregationResult :75-89); per doc the work is "set bit dictId" behind the filter -- scan_hist_kernel's loop
// (pg_scan_hist.h) with an OR where the histogram has an add.  The bitset IS the result: the host popcounts it.
//
// Two tiers, one body:
//   kLds = true   every DISTINCTCOUNT column (up to kMaxAggCols) keeps a bitset in the workgroup's dynamic LDS, side by side from
//                 word 0; one non-returning workgroup-scope OR of (match bit << (dictId & 31)) per doc -- unconditional, as the
//                 histogram's add is: a doc that does not match ORs zero.  At the end every workgroup ORs its non-zero words into
//                 the query's bitset in HBM (device-scope atomicOr, result unused).  One column alone reaches ~1.2 M dictIds.
//                 Measured against "plain LDS read, OR only where the bit is missing" (PG_DISTINCT_LDS_SKIP=1):
//                 0.597 ms against 0.639 ms on C2b-distinct at 1 B rows -- the unconditional OR is the form kept.
//                 This tier TRUSTS the forward index, as scan_hist_kernel does with its counters: a dictId at or above the
//                 cardinality (a corrupt segment) indexes past its column's bitset, into a neighbouring bitset or the filter's set
//                 area of the same workgroup's LDS -- a wrong answer for that query, never a write outside the workgroup's LDS
//                 allocation's hardware bounds.  The HBM tiers, where a stray index would leave the allocation, keep room for it.
//   kLds = false  test-then-OR straight into the zeroed bitset in HBM: a plain load of the word first (a stale copy can only
//                 say "not set", never the opposite: bits are never cleared during the launch), the atomic only when the bit is
//                 missing -- global atomics execute at the memory side and drop the line from L2, plain probes stay in it.
//                 Any cardinality up to 31-bit dictIds; PINOT_GPU_DISTINCT_LDS=0 sends every query here.
//   kGroup        (HBM only) the raw group id of each matching doc from the key columns' dictIds -- the arithmetic of
//                 group_private_kernel: sum dictId_j * mult_j -- selects row g of a [groups x words] bit matrix per column.
//
// Count and filter entries travel in the workgroups' records exactly as scan_hist_body's do (publish_block_partial).
#pragma once
#include "pg_kernels.h"
#include "pg_group_rows.h"      // distinct_rows16: the raw group ids of group_distinct_kernel (shared with pg_scan_counts.h)

namespace pg {

#ifndef PG_DISTINCT_LDS_SKIP
#define PG_DISTINCT_LDS_SKIP 0      // 1: the LDS tier reads the word and skips the OR when the bit is there (A/B builds: make variant DEFS=-DPG_DISTINCT_LDS_SKIP=1)
#endif

// Sixteen docs (half H) of the lane's chunk of one DISTINCTCOUNT column.  rows: kGroup -- the docs' raw group ids.
template <bool kLds, bool kGroup, int H>
__device__ __forceinline__ void distinct16(int b, const uint32_t* __restrict__ lane_words, uint32_t m, uint32_t* set_bits, int words, const uint32_t (&rows)[16]) {
  uint32_t v[16];
  decode16_private_dispatch<H>(b, lane_words, v);
  if constexpr (kLds) {
#if PG_DISTINCT_LDS_SKIP
    // the measured alternative: a plain LDS read first, the OR only where the bit is still missing
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = set_bits[v[j] >> 5];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t bit = __builtin_amdgcn_ubfe(m, 16 * H + j, 1) << (v[j] & 31u);
      if ((bit & ~w[j]) != 0u) __hip_atomic_fetch_or(set_bits + (v[j] >> 5), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
#else
#pragma unroll
    for (int j = 0; j < 16; ++j)
      __hip_atomic_fetch_or(set_bits + (v[j] >> 5), __builtin_amdgcn_ubfe(m, 16 * H + j, 1) << (v[j] & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (((m >> (16 * H + j)) & 1u) == 0u) continue;
      uint32_t* const w = set_bits + (kGroup ? (size_t)rows[j] * (size_t)words : (size_t)0) + (v[j] >> 5);
      const uint32_t bit = 1u << (v[j] & 31u);
      if ((*w & bit) == 0u) atomicOr(w, bit);
    }
  }
}

template <bool kLds, bool kGroup>
__device__ __forceinline__ void scan_distinct_body(const DistinctParams& dp, uint32_t* lds) {
  static_assert(!(kLds && kGroup), "the bit matrix of a group-by lives in HBM");
  const ScanParams& p = dp.scan;
  const int lane = threadIdx.x & 63;
  const int wave_in_block = threadIdx.x >> 6;
  const int waves_per_block = blockDim.x >> 6;
  const long long total_waves = (long long)gridDim.x * waves_per_block;
  const long long num_tiles = ((long long)p.num_docs + 2047) / 2048;
  if constexpr (kLds) for (int w = threadIdx.x; w < dp.lds_words; w += blockDim.x) lds[w] = 0u;
  // the filter's dictId sets behind the bitsets (set_leaves_in_lds = 1 + the area's byte offset, as scan_hist_body)
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
        distinct16<kLds, kGroup, 0>(col.bits, words, m, target, col.words, rows0);
        distinct16<kLds, kGroup, 1>(col.bits, words, m, target, col.words, rows1);
      }
    }
  }

  if constexpr (kLds) {
    // the workgroup's bitsets -> the query's: only the words that hold a bit
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kMaxAggCols; ++c) {
      if (c >= dp.num_cols) break;
      const DistinctCol& col = dp.cols[c];
      for (int w = threadIdx.x; w < col.words; w += blockDim.x) {
        const uint32_t bits = lds[col.lds_off + w];
        if (bits != 0u) atomicOr(col.set_bits + w, bits);
      }
    }
  }

  flush_filter_entries(p, entries);
  BlockPartial mine;
  partial_identity(mine);
  mine.count = (unsigned long long)wave_sum_i64((long long)count);
  mine.entries = (unsigned long long)wave_sum_i64((long long)entries);
  __syncthreads();       // every thread is done with the bitsets: the start of LDS becomes the reduction scratch
  BlockPartial* red = reinterpret_cast<BlockPartial*>(lds);
  if (lane == 0) red[wave_in_block] = mine;
  __syncthreads();
  publish_block_partial(p, red, waves_per_block, reinterpret_cast<uint32_t*>(red + waves_per_block), blockIdx.x, gridDim.x);      // (the engine sizes the LDS for it)
}

template <bool kLds>
__global__ __launch_bounds__(kLds ? kHistBlockThreads : kDistinctBlockThreads) void scan_distinct_kernel(const DistinctParams dp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t distinct_lds[];      // the only LDS object: bit addresses need no base add
  scan_distinct_body<kLds, false>(dp, distinct_lds);
}

__global__ __launch_bounds__(kDistinctBlockThreads) void group_distinct_kernel(const DistinctParams dp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t distinct_lds[];
  scan_distinct_body<false, true>(dp, distinct_lds);
}

}  // namespace pg
