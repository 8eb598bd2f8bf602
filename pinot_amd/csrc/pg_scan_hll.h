// scan_hll_kernel / group_hll_kernel / hll_fold_kernel / hll_pack_kernel: DISTINCTCOUNTHLL as HyperLogLog registers built on the device.
//
// What it replaces: DistinctCountHLLAggregationFunction.aggregate / aggregateGroupBySV -- on a raw column every matching doc's value is offered to
// the sketch, on a dictionary column the dictIds go into a RoaringBitmap first and the bitmap turns into the sketch once per segment
// (convertToHyperLogLog).  The arithmetic is pg_hll.h's; a register is the largest rank offered to it, so every update is a max, and
// registers are staged as 32-bit words here so that the max is one native LDS or global atomic.
//
// Raw columns, one pass, no sort (scan_hll_kernel): the body is scan_collect_body's -- the lane-private filter over 2048-doc tiles, a lane
// holding the match mask m of its 32 consecutive docs, the values read as stored (big-endian, sixteen bytes per load, eight-doc pieces
// without a match skipped).  Every slot (a column with a log2m, up to kMaxAggCols) keeps 2^log2m registers in the workgroup's dynamic LDS.
// Per matching doc: hash, read the register PLAINLY, issue the LDS max only when the rank is larger.  A stale read can only say "smaller"
// (registers never decrease during the launch), so the test never loses an update; after the first tiles almost no doc updates, which keeps
// 64 lanes off 2^log2m hot addresses.  At the end every workgroup max-merges its non-zero registers into the query's zeroed row in HBM.
// group_hll_kernel: the docs' raw group ids (distinct_rows16) select row g of a zeroed [rows x 2^log2m] matrix in HBM; the update is the same
// plain load, then atomicMax only where the rank is larger.
//
// Dictionary columns (hll_fold_kernel): scan_distinct_kernel / group_distinct_kernel run unchanged; the fold walks the rows of their bitsets,
// takes the dictionary value of every set bit from the device copy, hashes it and takes the max into the row's registers -- in LDS per
// workgroup, merged into the zeroed register row in HBM.  A workgroup whose words hold no bit touches nothing.
//
// hll_pack_kernel packs the staged words to bytes: only bytes cross the bus.
//
// Count and filter entries travel in the workgroups' records exactly as scan_collect_body's do (publish_block_partial).
#pragma once
#include "pg_kernels.h"
#include "pg_group_rows.h"
#include "pg_hll.h"

namespace pg {

// One offer: the register of hash x takes rank(x) when it is larger.  kLds: workgroup-scope LDS atomic, else device scope in HBM.
template <bool kLds>
__device__ __forceinline__ void hll_offer(uint32_t* __restrict__ row_regs, int log2m, uint64_t value) {
  const uint32_t x = hll_hash_long(value);
  uint32_t* const reg = row_regs + hll_index(x, log2m);
  const uint32_t rank = hll_rank(x, log2m);
  if (*reg < rank) {
    if constexpr (kLds) __hip_atomic_fetch_max(reg, rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else atomicMax(reg, rank);
  }
}

// The lane's 32 docs of one raw column.  rows: kGroup -- the docs' raw group ids (0..15, 16..31); a row at or above num_rows updates nothing.
template <bool kGroup, bool kWide>
__device__ __forceinline__ void hll_raw(const uint8_t* __restrict__ fwd, long long tile, int lane, uint32_t m, uint32_t* __restrict__ regs, int log2m,
                                        const uint32_t (&rows0)[16], const uint32_t (&rows1)[16], uint32_t num_rows) {
  const uint4* src = reinterpret_cast<const uint4*>(fwd + (tile * 2048 + (long long)lane * 32) * (kWide ? 8 : 4));
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t mc = (m >> (c * 8)) & 0xFFu;
    if (mc == 0u) continue;
    uint64_t v[8];
    if constexpr (kWide) {
      uint4 w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = src[c * 4 + i];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[2 * i] = ((uint64_t)__builtin_bswap32(w[i].x) << 32) | (uint64_t)__builtin_bswap32(w[i].y);
        v[2 * i + 1] = ((uint64_t)__builtin_bswap32(w[i].z) << 32) | (uint64_t)__builtin_bswap32(w[i].w);
      }
    } else {
      const uint4 w0 = src[c * 2], w1 = src[c * 2 + 1];
      const uint32_t dw[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = hll_long_of_bits32(__builtin_bswap32(dw[j]));
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (((mc >> j) & 1u) == 0u) continue;
      if constexpr (kGroup) {
        const uint32_t row = c < 2 ? rows0[c * 8 + j] : rows1[(c - 2) * 8 + j];
        if (row < num_rows) hll_offer<false>(regs + ((size_t)row << log2m), log2m, v[j]);
      } else {
        hll_offer<true>(regs, log2m, v[j]);
      }
    }
  }
}

template <bool kGroup>
__device__ __forceinline__ void scan_hll_body(const HllParams& hp, uint32_t* lds) {
  const DistinctParams& dp = hp.d;
  const ScanParams& p = dp.scan;
  const int lane = threadIdx.x & 63;
  const int wave_in_block = threadIdx.x >> 6;
  const int waves_per_block = blockDim.x >> 6;
  const long long total_waves = (long long)gridDim.x * waves_per_block;
  const long long num_tiles = ((long long)p.num_docs + 2047) / 2048;
  if constexpr (!kGroup) for (int w = threadIdx.x; w < hp.lds_words; w += blockDim.x) lds[w] = 0u;
  // the filter's dictId sets behind the registers (set_leaves_in_lds = 1 + the area's byte offset, as scan_hist_body)
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
        uint32_t* const target = kGroup ? hp.regs[c] : lds + hp.lds_off[c];
        if (hp.wide[c]) hll_raw<kGroup, true>(hp.fwd[c], tile, lane, m, target, hp.log2m[c], rows0, rows1, hp.num_rows);
        else hll_raw<kGroup, false>(hp.fwd[c], tile, lane, m, target, hp.log2m[c], rows0, rows1, hp.num_rows);
      }
    }
  }

  if constexpr (!kGroup) {
    // the workgroup's registers -> the query's: only the registers that hold a rank, and only where the query's is smaller
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kMaxAggCols; ++c) {
      if (c >= dp.num_cols) break;
      const int m_regs = 1 << hp.log2m[c];
      for (int j = threadIdx.x; j < m_regs; j += blockDim.x) {
        const uint32_t rank = lds[hp.lds_off[c] + j];
        if (rank != 0u && hp.regs[c][j] < rank) atomicMax(hp.regs[c] + j, rank);
      }
    }
  }

  flush_filter_entries(p, entries);
  BlockPartial mine;
  partial_identity(mine);
  mine.count = (unsigned long long)wave_sum_i64((long long)count);
  mine.entries = (unsigned long long)wave_sum_i64((long long)entries);
  __syncthreads();       // every thread is done with the registers and the staged sets: the start of LDS becomes the reduction scratch
  BlockPartial* red = reinterpret_cast<BlockPartial*>(lds);
  if (lane == 0) red[wave_in_block] = mine;
  __syncthreads();
  publish_block_partial(p, red, waves_per_block, reinterpret_cast<uint32_t*>(red + waves_per_block), blockIdx.x, gridDim.x);      // (the engine sizes the LDS for it)
}

__global__ __launch_bounds__(kHistBlockThreads) void scan_hll_kernel(const HllParams hp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hll_lds[];      // the only LDS object
  scan_hll_body<false>(hp, hll_lds);
}

__global__ __launch_bounds__(kDistinctBlockThreads) void group_hll_kernel(const HllParams hp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hll_lds[];
  scan_hll_body<true>(hp, hll_lds);
}

// ---- dictionary columns: bitset rows -> register rows ----
constexpr int kHllFoldThreads = 256;

__device__ __forceinline__ uint64_t hll_dict_long(const HllFoldParams& fp, uint32_t d) {
  switch (fp.dict_kind) {
    case kHllDictI32: return (uint64_t)((long long)fp.dict32[d] + fp.base);
    case kHllDictI64: return (uint64_t)fp.dict64[d];
    case kHllDictFloat: return hll_long_of_bits32(hll_float_bits_of_widened((uint64_t)fp.dict64[d]));
    default: return (uint64_t)fp.dict64[d];      // kHllDictDouble: doubleToRawLongBits
  }
}

__global__ __launch_bounds__(kHllFoldThreads) void hll_fold_kernel(const HllFoldParams fp) {
  extern __shared__ __attribute__((aligned(16))) uint32_t fold_regs[];      // [2^log2m]
  const long long row = (long long)(blockIdx.x / (unsigned)fp.chunks);
  const int chunk = (int)(blockIdx.x % (unsigned)fp.chunks);
  const int w_first = chunk * fp.words_per_chunk, w_end = min(fp.words, w_first + fp.words_per_chunk);
  const uint32_t* bits = fp.bits + row * (long long)fp.words;
  // a dictId at or above the cardinality has no dictionary entry: its bit (there is none in a sound segment) is masked off
  auto word_at = [&](int w) -> uint32_t {
    const int below = fp.cardinality - w * 32;
    if (below <= 0) return 0u;
    const uint32_t valid = below >= 32 ? 0xFFFFFFFFu : ((1u << below) - 1u);
    return bits[w] & valid;
  };
  uint32_t any = 0u;
  for (int w = w_first + (int)threadIdx.x; w < w_end; w += kHllFoldThreads) any |= word_at(w);
  if (__syncthreads_or((int)(any != 0u)) == 0) return;      // (uniform: no bit in this workgroup's words)
  const int m_regs = 1 << fp.log2m;
  for (int j = threadIdx.x; j < m_regs; j += kHllFoldThreads) fold_regs[j] = 0u;
  __syncthreads();
  for (int w = w_first + (int)threadIdx.x; w < w_end; w += kHllFoldThreads) {
    uint32_t word = word_at(w);
    while (word != 0u) {
      const uint32_t d = (uint32_t)w * 32u + (uint32_t)__builtin_ctz(word);
      word &= word - 1u;
      hll_offer<true>(fold_regs, fp.log2m, hll_dict_long(fp, d));
    }
  }
  __syncthreads();
  uint32_t* const out = fp.regs + ((size_t)row << fp.log2m);
  for (int j = threadIdx.x; j < m_regs; j += kHllFoldThreads) {
    const uint32_t rank = fold_regs[j];
    if (rank != 0u && out[j] < rank) atomicMax(out + j, rank);
  }
}

// n words (a multiple of four) -> n bytes: a register never exceeds 32 - log2m + 1.
__global__ __launch_bounds__(256) void hll_pack_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, unsigned long long n4) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (unsigned long long)gridDim.x * blockDim.x) {
    const uint4 w = reinterpret_cast<const uint4*>(in)[i];
    out[i] = (w.x & 0xFFu) | ((w.y & 0xFFu) << 8) | ((w.z & 0xFFu) << 16) | ((w.w & 0xFFu) << 24);
  }
}

}  // namespace pg
