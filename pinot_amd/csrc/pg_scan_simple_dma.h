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
#include "pg_dma_pairs.h"
#include "pg_scan_simple.h"

namespace pg {

typedef const __attribute__((address_space(3))) uint32_t* LdsWords;

// Dynamic LDS of a workgroup: the reduction records and the fold flag first (ONE LDS object: a second one beside a DMA target makes the
// compiler drain vmcnt(0) before LDS reads), then `waves` rings of `slots` slots of 256 * (f.bits + v.bits) bytes: kDmaRecordBytes,
// dma_slot_bytes and dma_lds_bytes of pg_dma_pairs.h.
static_assert(sizeof(BlockPartial) * (kBlockThreads / 64) + 16 <= kDmaRecordBytes, "the records and the flag fit their area");
static_assert(kDmaMaxBits == kSimpleMaxBits && kDmaWavesPerBlock == kBlockThreads / 64, "pg_dma_pairs.h speaks of this kernel's widths and workgroups");

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

// ------------------------------------------------------------------------------------------------
// scan_simple_dma_pair_kernel<FB, VB, kAux>: the same ring with the two widths as compile-time constants, for the pairs the rule admits
// (dma_pair_admitted).  Ownership, slots, the order of prologue, loop and drain, the lgkmcnt(0) in front of a slot's restaging, the counted
// vmcnt, the accumulators, the tail mask, the records and the fold are scan_simple_dma_body's; the per-value code is decode16_private /
// shift_in_lt / the umul24 sum.  What differs is the instruction path of a tile:
//     staging   which of the ceil(FB / 4) + ceil(VB / 4) instructions belongs to which column, its offset (an instruction immediate) and the
//               lanes of each column's last piece are constants: no select, at most two narrowed exec masks per tile
//     decode    no width switch; the lane's FB + VB dwords are all read from the slot at the top of the tile, f's first, and f is decoded
//               while v's reads are still landing (the compiler counts lgkmcnt down: nothing else in the loop uses that counter)
//     branches  lo == 0 and "the sum alone" (the headline's functions) are taken once around the tile loop; every other set of functions runs
//               the loop that keeps the sum, the minimum and the maximum, and what the query did not ask for is put back to its identity
//               behind the loop; an exclusive leaf is an xor with a uniform word
// Bit exact with scan_simple_dma_kernel and scan_simple_kernel.
// ------------------------------------------------------------------------------------------------
// Piece J of a column of B bits: 1 KiB from `src` (the chunk's first byte + lane * 16) to `dst` (the chunk's place in the slot).  The
// instruction's immediate offset moves both addresses; it reaches 4095, so a fifth piece starts from a second base.
template <int B, int J, int kAux>
__device__ __forceinline__ void dma_stage_piece(const uint8_t* src, uint8_t* dst, int lane) {
  constexpr int base = J >= 4 ? 4096 : 0, off = (J & 3) * 1024;
  if (J + 1 < dma_pieces(B) || dma_last_lanes(B) == 64 || lane < dma_last_lanes(B))
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + base), (__attribute__((address_space(3))) void*)(dst + base), 16, off, kAux);
}
template <int B, int kAux>
__device__ __forceinline__ void dma_stage_column(const uint8_t* src, uint8_t* dst, int lane) {
  static_assert(dma_pieces(B) <= 5, "columns of up to 20 bits");
  dma_stage_piece<B, 0, kAux>(src, dst, lane);
  if constexpr (dma_pieces(B) > 1) dma_stage_piece<B, 1, kAux>(src, dst, lane);
  if constexpr (dma_pieces(B) > 2) dma_stage_piece<B, 2, kAux>(src, dst, lane);
  if constexpr (dma_pieces(B) > 3) dma_stage_piece<B, 3, kAux>(src, dst, lane);
  if constexpr (dma_pieces(B) > 4) dma_stage_piece<B, 4, kAux>(src, dst, lane);
}

// One tile from its slot.  kMinMax: the minimum and the maximum beside the sum.  flip: ~0 for an exclusive leaf.
template <int FB, int VB, bool kLoZero, bool kMinMax>
__device__ __forceinline__ void dma_pair_tile(const uint8_t* slot, int lane, uint32_t lo, uint32_t span, uint32_t flip, long long rem,
                                              unsigned long long& count, unsigned long long& sum, uint32_t& umin, uint32_t& umax) {
  const LdsWords fw = (LdsWords)(const uint32_t*)slot + lane * FB;
  const LdsWords vw = (LdsWords)(const uint32_t*)(slot + 256 * FB) + lane * VB;
  uint32_t fd[FB], vd[VB];      // every dword once, all reads issued before the first is used
#pragma unroll
  for (int i = 0; i < FB; ++i) fd[i] = fw[i];
#pragma unroll
  for (int i = 0; i < VB; ++i) vd[i] = vw[i];
  uint32_t m = 0;
  range16_private<FB, 0, kLoZero>((const uint32_t*)fd, lo, span, m);
  range16_private<FB, 1, kLoZero>((const uint32_t*)fd, lo, span, m);
  m = __builtin_bitreverse32(m) ^ flip;      // value j -> bit j
  m &= rem >= 32 ? 0xFFFFFFFFu : (rem <= 0 ? 0u : ((1u << (int)rem) - 1u));        // docs past numDocs (last tile only)
  count += (unsigned)__builtin_popcount(m);
  uint32_t psum = 0, tmin = 0xFFFFFFFFu, tmax = 0u;
  unsigned long long wsum = 0;
  agg16_private<VB, 0>((const uint32_t*)vd, m, true, kMinMax, psum, wsum, tmin, tmax);
  agg16_private<VB, 1>((const uint32_t*)vd, m, true, kMinMax, psum, wsum, tmin, tmax);
  sum += wsum + psum;
  umin = tmin < umin ? tmin : umin;
  umax = tmax > umax ? tmax : umax;
}

// The wave's tiles first + k * total_waves, k < n, through its two slots: tile 0 staged ahead (the prologue); then, per tile, the next one
// staged into the other slot behind lgkmcnt(0) and vmcnt(N) -- or, for the last tile (the drain), vmcnt(0) alone -- and the decode.
template <int FB, int VB, int kAux, bool kLoZero, bool kMinMax, typename P>
__device__ __forceinline__ void dma_pair_tiles(const P& p, long long first, uint32_t n, long long total_waves, uint8_t* ring, int lane,
                                               unsigned long long& count, unsigned long long& sum, uint32_t& umin, uint32_t& umax) {
  constexpr int f_bytes = 256 * FB, v_bytes = 256 * VB, slot_bytes = f_bytes + v_bytes, N = dma_instructions(FB, VB);
  const auto& L = p.nodes[0];
  const uint32_t lo = (uint32_t)L.lo, span = L.span, flip = L.exclusive ? 0xFFFFFFFFu : 0u;
  const uint32_t lane_at = (uint32_t)lane * 16u;
  const uint8_t* f_next = L.fwd + first * f_bytes;              // the chunks of the tile to stage next: advance by adds
  const uint8_t* v_next = p.agg_cols[0].fwd + first * v_bytes;
  const long long f_step = total_waves * f_bytes, v_step = total_waves * v_bytes;
  long long rem = (long long)p.num_docs - (first * 2048 + lane * 32);
  const long long rem_step = total_waves * 2048;
  if (n > 0) {
    dma_stage_column<FB, kAux>(f_next + lane_at, ring, lane);
    dma_stage_column<VB, kAux>(v_next + lane_at, ring + f_bytes, lane);
  }
  int rd = 0;      // slot of tile i; the other one takes tile i + 1
  for (uint32_t i = 0; i < n; ++i, rem -= rem_step) {      // (n < 2^20: numDocs is a 32-bit count)
    if (i + 1 < n) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the other slot was read in the iteration before: those reads have returned
      f_next += f_step; v_next += v_step;
      uint8_t* wr = ring + (slot_bytes - rd);
      dma_stage_column<FB, kAux>(f_next + lane_at, wr, lane);
      dma_stage_column<VB, kAux>(v_next + lane_at, wr + f_bytes, lane);
      dma_wait<N>();
    } else {
      dma_wait<0>();
    }
    dma_pair_tile<FB, VB, kLoZero, kMinMax>(ring + rd, lane, lo, span, flip, rem, count, sum, umin, umax);
    rd = slot_bytes - rd;
  }
}

// p.nodes[0]: the range leaf of FB bits; p.agg_cols[0]: the aggregated column of VB bits.  lds: dma_lds_bytes(FB, VB, 2, blockDim.x / 64) bytes.
template <int FB, int VB, int kAux, typename P>
__device__ __forceinline__ void scan_simple_dma_pair_body(const P& p, uint32_t block_index, uint32_t num_blocks, uint8_t* lds) {
  static_assert(kDmaSlotsPerWave == 2 && dma_instructions(FB, VB) <= 63, "two slots; vmcnt counts to 63");
  BlockPartial* red = reinterpret_cast<BlockPartial*>(lds);
  uint32_t* fold_flag_ptr = reinterpret_cast<uint32_t*>(lds + sizeof(BlockPartial) * (kBlockThreads / 64));
  const int lane = threadIdx.x & 63;
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (uniform: the tile, its bases and the slot are scalars)
  const int waves_per_block = blockDim.x >> 6;
  const long long total_waves = (long long)num_blocks * waves_per_block;
  const long long num_tiles = ((long long)p.num_docs + 2047) / 2048;
  uint8_t* ring = lds + kDmaRecordBytes + (size_t)wave_in_block * kDmaSlotsPerWave * dma_slot_bytes(FB, VB);

  unsigned long long count = 0, sum = 0;
  uint32_t umin = 0xFFFFFFFFu, umax = 0u;
  const long long first = (long long)block_index * waves_per_block + wave_in_block;
  const uint32_t n = first < num_tiles ? (uint32_t)((num_tiles - first + total_waves - 1) / total_waves) : 0u;
  // the launch's uniform branches, once around the tile loop
  const bool lo_zero = p.nodes[0].lo == 0, need_sum = p.agg_cols[0].need_sum != 0, need_minmax = p.agg_cols[0].need_minmax != 0;
#define PG_PAIR_TILES(Z, M) dma_pair_tiles<FB, VB, kAux, Z, M>(p, first, n, total_waves, ring, lane, count, sum, umin, umax)
  if (lo_zero) { if (need_sum && !need_minmax) PG_PAIR_TILES(true, false); else PG_PAIR_TILES(true, true); }
  else { if (need_sum && !need_minmax) PG_PAIR_TILES(false, false); else PG_PAIR_TILES(false, true); }
#undef PG_PAIR_TILES
  if (!need_sum) sum = 0;      // (what scan_simple_dma_body leaves where the function was not asked for)
  if (!need_minmax) { umin = 0xFFFFFFFFu; umax = 0u; }

  BlockPartial mine;
  partial_identity(mine);
  mine.count = (unsigned long long)wave_sum_i64((long long)count);
  mine.sum[0] = wave_sum_i64((long long)sum);
  // unsigned keys below 2^31 -> the int32 keys of BlockPartial; lanes that matched nothing keep the identities
  mine.kmin[0] = wave_min_i32(umin == 0xFFFFFFFFu ? 0x7FFFFFFF : (int32_t)umin);
  mine.kmax[0] = wave_max_i32(count == 0ull ? (int32_t)0x80000000 : (int32_t)umax);
  if (lane == 0) red[wave_in_block] = mine;
  __syncthreads();      // (every DMA of this wave has landed: its last tile waited for vmcnt(0))
  publish_block_partial(p, red, waves_per_block, fold_flag_ptr, block_index, num_blocks);
}

// (scan_simple_dma_kernel<N, kAux> itself is defined in pg_unit_scan_simple_dma.hip, scan_simple_dma_pair_kernel<FB, VB, kAux> in
// pg_scan_simple_dma_pair_part.h: its instances are spread over kDmaPairParts units)

}  // namespace pg
