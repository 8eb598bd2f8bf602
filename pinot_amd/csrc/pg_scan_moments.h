// scan_moments_kernel / group_moments_kernel: the second run of VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP -- the pivoted moments
// S1 = sum(x - c) and S2 = sum((x - c)^2) of the matching docs' values.
//
// What it replaces: VarianceAggregationFunction.aggregate / aggregateGroupBySV (core/query/aggregation/function/VarianceAggregationFunction.java:
// 77-126) -- every matching doc's value goes through VarianceTuple.apply(double) (segment-local customobject/VarianceTuple.java:35-42), one
// division per doc, whose m2 loses its digits when the values sit far from zero.  Here the ordinary query has already brought count and sum; the
// pivot c = sum / count is the group's own mean up to SUM's rounding, so x - c is small where the values are close together, S2 is a sum of
// non-negative terms, and m2 = S2 - S1^2 / n corrects for what c misses of the mean (the host takes it: pg_engine.hip, harvest_moments).
//
// The body is scan_hll_body's / scan_collect_body's: the lane-private filter over 2048-doc tiles, a lane holding the match mask m of its 32
// consecutive docs, lanes and pieces without a match loading nothing, tile_list for index-led filters, the filter's dictId sets staged in LDS.
// Up to kMaxAggCols columns per launch, each read where it is stored (moments_lane, the one value switch of both kernels):
//   raw INT / FLOAT / LONG / DOUBLE   big-endian, sixteen bytes per load, eight-doc pieces without a match skipped (hll_raw's reads);
//   dictionary columns                the dictIds decoded as pg_scan_distinct.h decodes them (a half of sixteen docs without a match skipped), then
//                                     the device copy of the dictionary: 32-bit entries + value_base, longs, or doubles (FLOAT widened at open).
//                                     A dictId at or above the cardinality (a corrupt segment) reads the last entry, never past the copy.
// The value becomes a double as StatisticalAggregationFunctionUtils.getValSet makes it: (double) of the int / long / float.
//
// scan_moments_kernel: every lane keeps S1 and S2 per column in registers, in the fixed order of its tiles and docs; the wavefront reduces them
// with the xor butterfly (wave_sum_f64), the workgroup adds its wavefronts' sums in wavefront order, and ONE {S1, S2} record per column leaves the
// workgroup for slot blockIdx.x of the scratch.  The host adds the records in workgroup order behind one copy.  No floating-point atomic is on this
// path: the same query on the same grid returns bit-identical moments run after run.
// group_moments_kernel: the docs' raw group ids (distinct_rows16) select row g of a zeroed [rows x cols] matrix of {S1, S2} in HBM, updated with
// agent-scope double atomics (the idiom of the grouped double sums in pg_kernels.h); the pivot of (g, column) is read from the uploaded array.  A
// row at or above num_rows updates nothing.  The ORDER of these additions is whatever the hardware makes it: the last bits of a grouped m2 may
// differ between two runs of the same query.
//
// Count and filter entries travel in the workgroups' records exactly as scan_collect_body's do (publish_block_partial).
#pragma once
#include "pg_kernels.h"
#include "pg_group_rows.h"

namespace pg {

__device__ __forceinline__ double moments_dict_value(const MomentsCol& col, uint32_t d) {
  const uint32_t last = (uint32_t)(col.cardinality - 1);
  d = d < last ? d : last;
  switch (col.source) {
    case kMomentsDictI32: return (double)((long long)col.dict32[d] + col.base);
    case kMomentsDictI64: return (double)(long long)col.dict64[d];
    default: return __longlong_as_double((long long)col.dict64[d]);      // kMomentsDictF64
  }
}

// The lane's 32 docs of one column: use(j, x) for every doc j (0..31) whose bit of m is set, in ascending j.
template <typename Use>
__device__ __forceinline__ void moments_lane(const MomentsCol& col, long long tile, int lane, uint32_t m, Use&& use) {
  if (col.source >= kMomentsDictI32) {
    const uint32_t* words = reinterpret_cast<const uint32_t*>(col.fwd + tile * (256ll * col.bits)) + lane * col.bits;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t mh = (m >> (h * 16)) & 0xFFFFu;
      if (mh == 0u) continue;
      uint32_t v[16];
      if (h == 0) decode16_private_dispatch<0>(col.bits, words, v); else decode16_private_dispatch<1>(col.bits, words, v);
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if ((mh >> j) & 1u) use(h * 16 + j, moments_dict_value(col, v[j]));
    }
    return;
  }
  const bool wide = col.source == kMomentsRawI64 || col.source == kMomentsRawF64;
  const uint4* src = reinterpret_cast<const uint4*>(col.fwd + (tile * 2048 + (long long)lane * 32) * (wide ? 8 : 4));
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t mc = (m >> (c * 8)) & 0xFFu;
    if (mc == 0u) continue;
    double x[8];
    if (wide) {
      uint4 w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = src[c * 4 + i];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long lo = (long long)(((uint64_t)__builtin_bswap32(w[i].x) << 32) | (uint64_t)__builtin_bswap32(w[i].y));
        const long long hi = (long long)(((uint64_t)__builtin_bswap32(w[i].z) << 32) | (uint64_t)__builtin_bswap32(w[i].w));
        x[2 * i] = col.source == kMomentsRawI64 ? (double)lo : __longlong_as_double(lo);
        x[2 * i + 1] = col.source == kMomentsRawI64 ? (double)hi : __longlong_as_double(hi);
      }
    } else {
      const uint4 w0 = src[c * 2], w1 = src[c * 2 + 1];
      const uint32_t dw[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t bits = __builtin_bswap32(dw[j]);
        x[j] = col.source == kMomentsRawI32 ? (double)(int32_t)bits : (double)__uint_as_float(bits);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if ((mc >> j) & 1u) use(c * 8 + j, x[j]);
  }
}

template <bool kGroup>
__device__ __forceinline__ void scan_moments_body(const MomentsParams& mp, uint32_t* lds) {
  const DistinctParams& dp = mp.d;
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

  double s1[kMaxAggCols], s2[kMaxAggCols];
#pragma unroll
  for (int c = 0; c < kMaxAggCols; ++c) { s1[c] = 0.0; s2[c] = 0.0; }
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
      uint32_t rows[32];
      if constexpr (kGroup) {
        distinct_rows16<0>(dp, tile, lane, *reinterpret_cast<uint32_t(*)[16]>(&rows[0]));
        distinct_rows16<1>(dp, tile, lane, *reinterpret_cast<uint32_t(*)[16]>(&rows[16]));
      }
#pragma unroll
      for (int c = 0; c < kMaxAggCols; ++c) {
        if (c >= dp.num_cols) break;
        if constexpr (kGroup) {
          moments_lane(mp.cols[c], tile, lane, m, [&](int j, double x) {
            const uint32_t row = rows[j];
            if (row >= mp.num_rows) return;
            const size_t cell = (size_t)row * (size_t)dp.num_cols + (size_t)c;
            const double d = x - mp.pivots[cell];
            __hip_atomic_fetch_add(mp.out + 2 * cell, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(mp.out + 2 * cell + 1, d * d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          });
        } else {
          const double pivot = mp.pivot[c];
          moments_lane(mp.cols[c], tile, lane, m, [&](int, double x) {
            const double d = x - pivot;
            s1[c] += d;
            s2[c] += d * d;
          });
        }
      }
    }
  }

  if constexpr (!kGroup) {
    // lane -> wavefront (the xor butterfly) -> workgroup (wavefront order) -> the workgroup's record: a fixed tree
    __syncthreads();       // every thread is done with the staged sets: the start of LDS holds the wavefronts' sums
    double* wave_sums = reinterpret_cast<double*>(lds);      // [waves_per_block][kMaxAggCols][2]
#pragma unroll
    for (int c = 0; c < kMaxAggCols; ++c) {
      if (c >= dp.num_cols) break;
      const double w1 = wave_sum_f64(s1[c]), w2 = wave_sum_f64(s2[c]);
      if (lane == 0) { wave_sums[(wave_in_block * kMaxAggCols + c) * 2] = w1; wave_sums[(wave_in_block * kMaxAggCols + c) * 2 + 1] = w2; }
    }
    __syncthreads();
    if ((int)threadIdx.x < dp.num_cols * 2) {
      const int c = (int)threadIdx.x >> 1, which = (int)threadIdx.x & 1;
      double acc = wave_sums[c * 2 + which];
      for (int w = 1; w < waves_per_block; ++w) acc += wave_sums[(w * kMaxAggCols + c) * 2 + which];
      mp.out[((size_t)blockIdx.x * (size_t)dp.num_cols + (size_t)c) * 2 + (size_t)which] = acc;
    }
  }

  flush_filter_entries(p, entries);
  BlockPartial mine;
  partial_identity(mine);
  mine.count = (unsigned long long)wave_sum_i64((long long)count);
  mine.entries = (unsigned long long)wave_sum_i64((long long)entries);
  __syncthreads();       // every thread is done with the staged sets and the wavefronts' sums: the start of LDS becomes the reduction scratch
  BlockPartial* red = reinterpret_cast<BlockPartial*>(lds);
  if (lane == 0) red[wave_in_block] = mine;
  __syncthreads();
  publish_block_partial(p, red, waves_per_block, reinterpret_cast<uint32_t*>(red + waves_per_block), blockIdx.x, gridDim.x);      // (the engine sizes the LDS for it)
}

constexpr int kMomentsBlockThreads = kDistinctBlockThreads;      // four wavefronts: the accumulators live in registers, LDS holds the staged sets and the records
static_assert(sizeof(double) * 2 * kMaxAggCols * (kMomentsBlockThreads / 64) <= sizeof(BlockPartial) * (kMomentsBlockThreads / 64), "the wavefronts' sums fit where the records go");

__global__ __launch_bounds__(kMomentsBlockThreads) void scan_moments_kernel(const MomentsParams mp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t moments_lds[];      // the only LDS object
  scan_moments_body<false>(mp, moments_lds);
}

__global__ __launch_bounds__(kMomentsBlockThreads) void group_moments_kernel(const MomentsParams mp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t moments_lds[];
  scan_moments_body<true>(mp, moments_lds);
}

}  // namespace pg
