// scan_simple_dma_kernel: scan_simple_pipe_kernel's queries -- ONE dictionary-range leaf AND one aggregated packed column, a filter that
// matches a tile's every chunk anyway -- with the two columns streamed through a wave-private ring of LDS slots by LDS-DMA loads.
//
// What the register kernels cannot change about their request shape: a lane reads its own `bits` consecutive dwords as
// dwordx4 loads at a 4 * bits byte stride, so every wave-instruction touches every line of the chunk and the L1 has to merge them; such
// loads cannot be non-temporal (each depends on a sibling's L1 hit); and a tile ahead costs its registers.  Here a tile's two chunks are
// fetched as whole 1 KiB pieces -- 64 lanes x 16 consecutive bytes per instruction, the last instruction of a chunk with the lanes its
// remainder needs -- straight into the wave's slot in LDS, S - 1 tiles ahead of the decode, and the lane then reads its own dwords from
// the slot:
//     prologue    stage tiles 0 .. S-2 into slots 0 .. S-2
//     iteration   stage tile i+S-1; s_waitcnt vmcnt(N * (S-1)): tile i has landed; decode f(i) -> mask, v(i) under the mask, from its slot
//     epilogue    the last S-1 tiles: counted waits, nothing issued
// N = the LDS-DMA instructions of a tile = ceil(f.bits / 4) + ceil(v.bits / 4), a template parameter: the wait's immediate.  The widths
// themselves are run-time values; no load sits behind a width switch.  Every load stays inside the wave's own tile: the kernel reads
// exactly the bytes scan_simple_kernel reads.  The slots are wave-private -- no barrier in the tile loop -- and the tile loop holds no
// ordinary global load (the parameters are scalar loads), so its only vmcnt waits are the counted ones.
//
// Same ownership (lane i: docs 32i .. 32i+31 of a 2048-doc tile), same per-value code (simple_range_dispatch / simple_agg_dispatch on an
// LDS pointer), same accumulators, tail mask and records as scan_simple_body: bit exact with it.
#pragma once
#include "pg_scan_simple.h"

namespace pg {

typedef const __attribute__((address_space(3))) uint32_t* LdsWords;

// Dynamic LDS of a workgroup: the reduction records and the fold flag first (ONE LDS object: a second one beside a DMA target makes the
// compiler drain vmcnt(0) before LDS reads), then `waves` rings of `slots` slots of 256 * (f.bits + v.bits) bytes.
constexpr int kDmaRecordBytes = 1024;
static_assert(sizeof(BlockPartial) * (kBlockThreads / 64) + 16 <= kDmaRecordBytes, "the records and the flag fit their area");
__host__ __device__ constexpr int dma_slot_bytes(int filter_bits, int value_bits) { return 256 * (filter_bits + value_bits); }
__host__ __device__ constexpr size_t dma_lds_bytes(int filter_bits, int value_bits, int slots, int waves) {
  return (size_t)kDmaRecordBytes + (size_t)waves * slots * dma_slot_bytes(filter_bits, value_bits);
}

template <int J> __device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(J) : "memory"); }

// One tile's two chunks into `slot` (f at 0, v at 256 * f.bits): N instructions, instruction j the (j - 0)-th KiB of f or the (j - nf)-th of
// v, by wave-uniform selects -- every one of the N is issued exactly once per tile (its first lanes are always inside the chunk).
template <int N, int kAux>
__device__ __forceinline__ void dma_stage_tile(const uint8_t* f_tile, const uint8_t* v_tile, int f_bytes, int v_bytes, int nf, uint8_t* slot, int lane) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const bool is_f = j < nf;
    const int at = (is_f ? j : j - nf) * 1024, chunk = is_f ? f_bytes : v_bytes;
    const uint8_t* src = (is_f ? f_tile : v_tile) + at + lane * 16;
    uint8_t* dst = slot + (is_f ? 0 : f_bytes) + at;
    if (at + lane * 16 < chunk)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, kAux);
  }
}

// One tile from its slot: scan_simple_body's tile, always aggregating (no lane skip, no sparse walk: the pipelined kernel's rule).
template <typename P>
__device__ __forceinline__ void dma_tile(const P& p, long long tile, int lane, const uint8_t* slot, unsigned long long& count, unsigned long long& sum,
                                         uint32_t& umin, uint32_t& umax) {
  const auto& L = p.nodes[0];
  const auto& ac = p.agg_cols[0];
  const LdsWords fw = (LdsWords)(const uint32_t*)slot + lane * L.bits;
  const LdsWords vw = (LdsWords)(const uint32_t*)(slot + 256 * L.bits) + lane * ac.bits;
  uint32_t m = L.lo == 0 ? simple_range_dispatch<true>(L.bits, fw, 0u, L.span) : simple_range_dispatch<false>(L.bits, fw, (uint32_t)L.lo, L.span);
  if (L.exclusive) m = ~m;
  const long long rem = (long long)p.num_docs - (tile * 2048 + lane * 32);        // docs past numDocs (last tile only)
  m &= rem >= 32 ? 0xFFFFFFFFu : (rem <= 0 ? 0u : ((1u << (int)rem) - 1u));
  count += (unsigned)__builtin_popcount(m);
  uint32_t psum = 0, tmin = 0xFFFFFFFFu, tmax = 0u;
  unsigned long long wsum = 0;
  simple_agg_dispatch(ac.bits, vw, m, ac.need_sum != 0, ac.need_minmax != 0, psum, wsum, tmin, tmax);
  sum += wsum + psum;
  umin = tmin < umin ? tmin : umin;
  umax = tmax > umax ? tmax : umax;
}

// p.nodes[0]: the range leaf; p.agg_cols[0]: the aggregated column; (f.bits + 3) / 4 + (v.bits + 3) / 4 == N (launch_scan_simple_dma).
// lds: dma_lds_bytes(f.bits, v.bits, S, blockDim.x / 64) bytes.
template <int N, int S, int kAux, typename P>
__device__ __forceinline__ void scan_simple_dma_body(const P& p, uint32_t block_index, uint32_t num_blocks, uint8_t* lds) {
  static_assert(S >= 2 && N * (S - 1) <= 63, "vmcnt counts to 63");
  BlockPartial* red = reinterpret_cast<BlockPartial*>(lds);
  uint32_t* fold_flag_ptr = reinterpret_cast<uint32_t*>(lds + sizeof(BlockPartial) * (kBlockThreads / 64));
  const int lane = threadIdx.x & 63;
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (uniform: the tile, its bases and the slot are scalars)
  const int waves_per_block = blockDim.x >> 6;
  const long long total_waves = (long long)num_blocks * waves_per_block;
  const long long num_tiles = ((long long)p.num_docs + 2047) / 2048;
  const auto& L = p.nodes[0];
  const auto& ac = p.agg_cols[0];
  const int f_bytes = 256 * L.bits, v_bytes = 256 * ac.bits, slot_bytes = f_bytes + v_bytes, nf = (L.bits + 3) >> 2;
  uint8_t* ring = lds + kDmaRecordBytes + (size_t)wave_in_block * S * slot_bytes;

  unsigned long long count = 0, sum = 0;
  uint32_t umin = 0xFFFFFFFFu, umax = 0u;
  const long long first = (long long)block_index * waves_per_block + wave_in_block;
  // the wave's tiles: first + k * total_waves, k < n
  const long long n = first < num_tiles ? (num_tiles - first + total_waves - 1) / total_waves : 0;
#pragma unroll
  for (int k = 0; k < S - 1; ++k)
    if (k < n) dma_stage_tile<N, kAux>(L.fwd + (first + k * total_waves) * f_bytes, ac.fwd + (first + k * total_waves) * v_bytes, f_bytes, v_bytes, nf, ring + k * slot_bytes, lane);
  long long i = 0, tile = first;
  int rd = 0, wr = S - 1;      // slot of tile i, slot of tile i + S - 1
  for (; i + (S - 1) < n; ++i, tile += total_waves) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // slot `wr` was read in the iteration before: those reads have returned
    const long long ahead = tile + (S - 1) * total_waves;
    dma_stage_tile<N, kAux>(L.fwd + ahead * f_bytes, ac.fwd + ahead * v_bytes, f_bytes, v_bytes, nf, ring + wr * slot_bytes, lane);
    dma_wait<N * (S - 1)>();
    dma_tile(p, tile, lane, ring + rd * slot_bytes, count, sum, umin, umax);
    rd = rd + 1 == S ? 0 : rd + 1;
    wr = wr + 1 == S ? 0 : wr + 1;
  }
  // the last min(n, S - 1) tiles are in flight and nothing follows them: r of them left -> r - 1 may stay out
#define PG_DMA_DRAIN(R) if (S - 1 >= R && n - i == R) { dma_wait<N * (R - 1)>(); dma_tile(p, tile, lane, ring + rd * slot_bytes, count, sum, umin, umax); \
                          rd = rd + 1 == S ? 0 : rd + 1; ++i; tile += total_waves; }
  PG_DMA_DRAIN(3) PG_DMA_DRAIN(2) PG_DMA_DRAIN(1)
#undef PG_DMA_DRAIN
  static_assert(S <= 4, "PG_DMA_DRAIN covers rings of up to four slots");

  BlockPartial mine;
  partial_identity(mine);
  mine.count = (unsigned long long)wave_sum_i64((long long)count);
  mine.sum[0] = wave_sum_i64((long long)sum);
  // unsigned keys below 2^31 -> the int32 keys of BlockPartial; lanes that matched nothing keep the identities
  mine.kmin[0] = wave_min_i32(umin == 0xFFFFFFFFu ? 0x7FFFFFFF : (int32_t)umin);
  mine.kmax[0] = wave_max_i32(count == 0ull ? (int32_t)0x80000000 : (int32_t)umax);
  if (lane == 0) red[wave_in_block] = mine;
  __syncthreads();      // (every DMA of this wave has landed: the drain above ends on vmcnt(0))
  publish_block_partial(p, red, waves_per_block, fold_flag_ptr, block_index, num_blocks);
}

// (scan_simple_dma_kernel<N, S, kAux> itself is defined in pg_unit_scan_simple_dma.hip)

}  // namespace pg
