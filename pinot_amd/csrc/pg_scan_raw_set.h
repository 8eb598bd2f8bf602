// The kernels of a PG_PRED_RAW_SET leaf -- `WHERE rawCol IN (...)` / `NOT IN (...)` on a raw (no-dictionary, PASS_THROUGH) INT / LONG /
// FLOAT / DOUBLE column.
//
// What they replace: ScanBasedFilterOperator + SVScanDocIdIterator with an Int / Long / Float / DoubleRawValueBasedInPredicateEvaluator
// (InPredicateEvaluatorFactory.java:74-107, :215-380: `set.contains(value)` on a fastutil open hash set; NotInPredicateEvaluatorFactory
// negates) over a FixedByteChunkSVForwardIndexReader.
//
// Membership: the host builds a table of four-slot buckets in which every key sits in its home bucket (pg_raw_set_table.h); a workgroup
// stages it into LDS once, and a doc's lookup is one hash, one bucket read (ds_read_b128; two for 8-byte keys) and four compares -- no
// probe loop, no branch.  Keys are compared in the column's on-disk (big-endian) byte order, so the filter column is never byte-swapped.
//
//  * scan_raw_set_kernel<4 | 8>  (tier 1) the sibling of scan_raw_kernel: the whole filter is ONE such leaf, at most one aggregated
//    column, and that column is a raw INT column.  Same coalesced 16-byte tile loads, tail masking, BlockPartial reduction and fold.
//  * raw_set_bitmap_kernel<4 | 8> (tier 2) everything else: reads the column once and leaves the leaf's doc-order match bitmap (one
//    dword per lane and tile, the format of a kLeafBitmap leaf), which every kernel family already evaluates.
#pragma once
#include "pg_raw_set_table.h"
#include "pg_scan_raw.h"

namespace pg {

#ifndef PG_RAW_SET_WAVES
#define PG_RAW_SET_WAVES 4              // wavefronts per SIMD the register allocation must allow (as scan_raw_kernel: PG_RAW_WAVES)
#endif

extern __shared__ raw_u32x4 raw_set_lds[];      // the table: bucket b of 4-byte keys = raw_set_lds[b], of 8-byte keys = raw_set_lds[2 b], [2 b + 1]

__device__ __forceinline__ void stage_raw_set_table(const uint32_t* table, uint32_t table_bytes) {
  const raw_u32x4* src = reinterpret_cast<const raw_u32x4*>(table);
  for (uint32_t i = threadIdx.x; i < table_bytes / 16; i += blockDim.x) raw_set_lds[i] = src[i];
  __syncthreads();
}
__device__ __forceinline__ uint32_t raw_set_hit32(uint32_t w, uint32_t mult, uint32_t shift) {
  const raw_u32x4 b = raw_set_lds[raw_set_bucket32(w, mult, shift)];
  return ((b.x == w) | (b.y == w) | (b.z == w) | (b.w == w)) ? 1u : 0u;
}
__device__ __forceinline__ uint32_t raw_set_hit64(uint32_t w0, uint32_t w1, uint32_t mult, uint32_t shift) {
  const uint32_t b = 2u * raw_set_bucket64(w0, w1, mult, shift);
  const raw_u32x4 lo = raw_set_lds[b], hi = raw_set_lds[b + 1];
  return (((lo.x == w0) & (lo.y == w1)) | ((lo.z == w0) & (lo.w == w1)) | ((hi.x == w0) & (hi.y == w1)) | ((hi.z == w0) & (hi.w == w1))) ? 1u : 0u;
}

// The docs a lane sees of a 2048-doc tile, and the bit each gets in the lane's 32-bit mask.  Every load instruction of a wave covers one
// contiguous kilobyte (16 bytes per lane), so:
//   4-byte keys  piece j (of 8) holds docs 256 j + 4 lane + k, k < 4: bit 4 j + k   (scan_raw_body's layout: RawTile)
//   8-byte keys  piece i (of 16) holds docs 128 i + 2 lane + k, k < 2: bit 2 i + k
// An aggregated raw INT column is read in the filter's layout: RawTile next to 4-byte keys, sixteen 8-byte pieces next to 8-byte keys.
typedef uint32_t raw_u32x2 __attribute__((ext_vector_type(2)));

template <int kKeyBytes>
__device__ __forceinline__ uint32_t raw_set_tile_mask(const uint8_t* fwd, long long tile, int lane, uint32_t mult, uint32_t shift, RawTile& t) {
  uint32_t m = 0u;
  if (kKeyBytes == 4) {
    load_raw_tile(fwd, tile, lane, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      m |= raw_set_hit32(t.q[j].x, mult, shift) << (4 * j);
      m |= raw_set_hit32(t.q[j].y, mult, shift) << (4 * j + 1);
      m |= raw_set_hit32(t.q[j].z, mult, shift) << (4 * j + 2);
      m |= raw_set_hit32(t.q[j].w, mult, shift) << (4 * j + 3);
    }
  } else {
    const raw_u32x4* base = reinterpret_cast<const raw_u32x4*>(fwd + tile * 16384) + lane;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int i = 0; i < 8; ++i) t.q[i] = __builtin_nontemporal_load(base + 64 * (8 * h + i));
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        m |= raw_set_hit64(t.q[i].x, t.q[i].y, mult, shift) << (2 * (8 * h + i));
        m |= raw_set_hit64(t.q[i].z, t.q[i].w, mult, shift) << (2 * (8 * h + i) + 1);
      }
    }
  }
  return m;
}
// clears the bits of docs past the segment's end (`rem`: docs of this tile that exist, fewer than 2048)
template <int kKeyBytes>
__device__ __forceinline__ uint32_t raw_set_tail_mask(uint32_t m, long long rem, int lane) {
  constexpr int kPieces = kKeyBytes == 4 ? 8 : 16, kDocs = 32 / kPieces;      // docs of a lane per piece: 4 | 2
#pragma unroll
  for (int j = 0; j < kPieces; ++j) {
    const long long left = rem - ((2048 / kPieces) * j + kDocs * lane);
    const uint32_t all = (1u << kDocs) - 1u;
    const uint32_t keep = left >= kDocs ? all : (left <= 0 ? 0u : ((1u << (int)left) - 1u));
    m &= ~(all << (kDocs * j)) | (keep << (kDocs * j));
  }
  return m;
}

// nodes[0]: fwd = the filter column, set_words / set_bytes = the table, lo = the hash multiplier, span = its shift, exclusive = NOT IN
template <int kKeyBytes>
__device__ __forceinline__ void scan_raw_set_body(const ScanParams& p, BlockPartial* red, uint32_t* fold_flag_ptr) {
  const int lane = threadIdx.x & 63;
  const int wave_in_block = threadIdx.x >> 6;
  const int waves_per_block = blockDim.x >> 6;
  const long long total_waves = (long long)gridDim.x * waves_per_block;
  const long long num_tiles = ((long long)p.num_docs + 2047) / 2048;
  const bool has_agg = p.num_agg_cols == 1;
  const auto& L = p.nodes[0];
  const auto& ac = p.agg_cols[0];
  const bool same_column = kKeyBytes == 4 && has_agg && L.fwd == ac.fwd;      // (then the tile is read once)
  const uint32_t mult = (uint32_t)L.lo, shift = L.span;
  const bool need_sum = has_agg && ac.need_sum != 0, need_minmax = has_agg && ac.need_minmax != 0;
  stage_raw_set_table(L.set_words, (uint32_t)L.set_bytes);

  unsigned long long count = 0;
  long long sum = 0;
  int32_t vmin = 0x7FFFFFFF, vmax = (int32_t)0x80000000;
  for (long long tile = (long long)blockIdx.x * waves_per_block + wave_in_block; tile < num_tiles; tile += total_waves) {
    const long long rem = (long long)p.num_docs - tile * 2048;           // docs of this tile that exist (the last tile: fewer than 2048)
    RawTile t;
    uint32_t m = raw_set_tile_mask<kKeyBytes>(L.fwd, tile, lane, mult, shift, t);
    if (L.exclusive) m = ~m;
    if (rem < 2048) m = raw_set_tail_mask<kKeyBytes>(m, rem, lane);
    count += (unsigned)__builtin_popcount(m);
    if (!has_agg) continue;
    if (!same_column && __builtin_amdgcn_ballot_w64(m != 0u) == 0ull) continue;      // nothing matched in the whole tile: the aggregated column is not read
    if (kKeyBytes == 4) {
      if (!same_column) load_raw_tile(ac.fwd, tile, lane, t);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool hit = ((m >> (4 * j + k)) & 1u) != 0u;
          const int32_t x = (int32_t)raw_value(t, j, k);
          if (need_sum) sum += hit ? (long long)x : 0ll;
          if (need_minmax) {
            vmin = (hit && x < vmin) ? x : vmin;
            vmax = (hit && x > vmax) ? x : vmax;
          }
        }
      }
    } else {
      // the INT column in the 8-byte layout: piece i = the wave's contiguous 512 bytes, two docs per lane
      const raw_u32x2* base = reinterpret_cast<const raw_u32x2*>(ac.fwd + tile * 8192) + lane;
      raw_u32x2 v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = __builtin_nontemporal_load(base + 64 * i);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const bool hit = ((m >> (2 * i + k)) & 1u) != 0u;
          const int32_t x = (int32_t)__builtin_bswap32(k == 0 ? v[i].x : v[i].y);
          if (need_sum) sum += hit ? (long long)x : 0ll;
          if (need_minmax) {
            vmin = (hit && x < vmin) ? x : vmin;
            vmax = (hit && x > vmax) ? x : vmax;
          }
        }
      }
    }
  }

  BlockPartial mine;
  partial_identity(mine);
  mine.count = (unsigned long long)wave_sum_i64((long long)count);
  mine.sum[0] = wave_sum_i64(sum);
  mine.kmin[0] = wave_min_i32(vmin);
  mine.kmax[0] = wave_max_i32(vmax);
  if (lane == 0) red[wave_in_block] = mine;
  __syncthreads();
  publish_block_partial(p, red, waves_per_block, fold_flag_ptr, blockIdx.x, gridDim.x);
}

// Tier 2: the same coalesced tile reads and lookups; the lanes' masks are then turned into doc-order dwords.  Dword w of a tile (docs
// 32 w .. 32 w + 31) is made of one piece's bits of a GROUP of consecutive lanes -- 4-byte keys: piece w / 8, the eight lanes 8 (w % 8) ..,
// four bits each; 8-byte keys: piece w / 4, the sixteen lanes 16 (w % 4) .., two bits each -- so a butterfly OR over the group (3 | 4
// exchanges per piece) leaves every piece's dword in all lanes of its group, and lane (group g, rank r) stores the dword of piece r:
// one dword per lane, the wave's 256 bytes of a tile in one store instruction.  Docs past num_docs (the column's zero padding) are
// cleared: 0 may be a member.
template <int kKeyBytes>
__device__ __forceinline__ void raw_set_bitmap_body(const RawSetBitmapParams& p) {
  constexpr int kPieces = kKeyBytes == 4 ? 8 : 16, kDocs = 32 / kPieces, kGroup = kPieces;      // lanes of a group = 32 docs / docs per lane and piece: 8 | 16, as many as pieces
  const int lane = threadIdx.x & 63;
  const int rank = lane & (kGroup - 1), group = lane / kGroup;
  const int waves_per_block = blockDim.x >> 6;
  const long long total_waves = (long long)gridDim.x * waves_per_block;
  const long long num_tiles = ((long long)p.num_docs + 2047) / 2048;
  stage_raw_set_table(p.table, p.table_bytes);
  for (long long tile = (long long)blockIdx.x * waves_per_block + (threadIdx.x >> 6); tile < num_tiles; tile += total_waves) {
    RawTile t;
    const uint32_t m = raw_set_tile_mask<kKeyBytes>(p.fwd, tile, lane, p.mult, p.shift, t);
    uint32_t mine = 0u;
#pragma unroll
    for (int j = 0; j < kPieces; ++j) {
      uint32_t v = ((m >> (kDocs * j)) & ((1u << kDocs) - 1u)) << (kDocs * rank);
#pragma unroll
      for (int x = 1; x < kGroup; x <<= 1) v |= (uint32_t)__shfl_xor((int)v, x);
      mine = rank == j ? v : mine;
    }
    // lane (group, rank) holds the dword of piece `rank`: docs (2048 / kPieces) rank + 32 group ..
    const int w = (kGroup == 8 ? 8 : 4) * rank + group;
    const long long left = (long long)p.num_docs - (tile * 2048 + 32 * w);
    const uint32_t keep = left >= 32 ? 0xFFFFFFFFu : (left <= 0 ? 0u : ((1u << (int)left) - 1u));
    p.out[tile * 64 + w] = mine & keep;
  }
}

// (the kernels themselves are defined in pg_unit_scan_raw_set.hip)

}  // namespace pg
