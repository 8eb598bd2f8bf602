// scan_simple_pipe_kernel: scan_simple_kernel's shape with ONE dictionary-range leaf AND one aggregated packed column, for filters that match
// a tile's every chunk anyway -- the loads of the two columns software-pipelined across tiles.
//
// scan_simple_body does, per tile and strictly in this order: load f, wait, decode f into the mask, load v, wait, decode v.  The v load waits
// for the mask because a lane without a match skips it (and a tile without one, and a tile with few walks its matches): what the 1-3 %
// filters live on.  At 10 % a lane's 32 docs hold no match with probability 0.9^32 = 3 % and a tile always holds one, so the order buys
// nothing there and costs two dependent round trips per tile, with nothing of the wave's in flight while it decodes.  Here:
//     prologue    load f(first tile)
//     iteration   issue v(i) and f(i+1) into register arrays; pin them; decode f(i) from registers -> mask, tail mask, popcount;
//                 decode v(i) under the mask; f(i+1) becomes f(i)
//     epilogue    the wave's last tile: issue v(i) alone, decode f(i) and v(i)
// -- a wave always has a chunk in flight while it decodes another, a tile costs one round trip, and the waits are counted (the f(i) decode
// waits for nothing this iteration issued, the v(i) decode not for f(i+1)).  No lane skip, no sparse walk, no `continue` on an empty tile:
// choose_scan_kernel sends the filters that want those to scan_simple_kernel (PINOT_GPU_SCAN_SIMPLE_PIPE).
//
// Same ownership (lane i: docs 32i .. 32i+31 of a 2048-doc tile, the `bits` dwords from i * bits), same per-value code (range16_private /
// agg16_private on the register array), same accumulators and tail as scan_simple_body: bit exact with it.
//
// The SHAPE of the loads is a compile-time property of the tile loop: loads whose count follows a run-time width through wave-uniform
// branches make the compiler drain vmcnt(0) at every join, which is the serialisation this kernel exists to remove.  So the loop is a
// template on the number of 16-byte loads per lane and column, <NF4, NV4> with N = ceil(bits / 4): 21 instantiations (<4, 5>, <5, 3>,
// <5, 4> and <5, 5> spill at five waves per SIMD: those pairs stay with scan_simple_kernel), each decoding the four widths of its class
// through a switch that touches registers only.
#pragma once
#include "pg_scan_simple.h"

namespace pg {

// A chunk is read as N x global_load_dwordx4 from the lane's first dword: up to 12 bytes more than the lane's own `bits` dwords.  Those
// bytes belong to the next lane, whose line the wave reads anyway -- except behind the tile's last lanes, where they would be the next
// tile's first line: another wave's, most often on another XCD (a second fetch of that line from memory), and past the column behind the
// last tile.  So a lane whose last load would cross its tile's end starts that load `back` dwords earlier (pipe_tail_back: lane 63 for
// most widths, lanes 61 to 63 at one bit) and moves the registers up before it decodes (pipe_align_tail).  No load leaves the wave's own
// tile: the kernel reads the bytes scan_simple_kernel reads, and needs no more of the allocation than the whole tiles that kernel needs.
static_assert((kSimpleMaxBits + 3) / 4 == 5, "scan_simple_pipe_kernel is instantiated for one to five 16-byte loads per column");

typedef uint32_t Dword4 __attribute__((ext_vector_type(4), aligned(4)));

template <int N4>
__device__ __forceinline__ int pipe_tail_back(int lane, int bits) {
  const int over = lane * bits + 4 * N4 - 64 * bits;      // dwords past the tile's end: at most 4 * N4 - bits <= 3
  return over > 0 ? over : 0;
}

// tile_words: the wave's tile (uniform: a scalar base); at: the lane's first dword in it; tail: where the lane's last load starts
template <int N4>
__device__ __forceinline__ void pipe_load_chunk(GlobalWords tile_words, uint32_t at, uint32_t tail, uint32_t (&r)[4 * N4]) {
#pragma unroll
  for (int i = 0; i < N4; ++i) {
    const Dword4 q = *(const __attribute__((address_space(1))) Dword4*)(i == N4 - 1 ? tile_words + tail : tile_words + at + 4 * i);
    r[4 * i + 0] = q.x; r[4 * i + 1] = q.y; r[4 * i + 2] = q.z; r[4 * i + 3] = q.w;
  }
}

// The last load of a lane that started it `back` dwords early holds dword 4 * (N4 - 1) + j - back in register j: move the 4 - K dwords
// the width has there up by `back` <= K.  (Registers only; the other lanes keep theirs.)
template <int N4, int K>
__device__ __forceinline__ void pipe_align_tail(uint32_t (&r)[4 * N4], int back) {
  constexpr int t = 4 * (N4 - 1);
  if (K >= 1) {
    const bool one = (back & 1) != 0;
    r[t + 0] = one ? r[t + 1] : r[t + 0]; r[t + 1] = one ? r[t + 2] : r[t + 1]; r[t + 2] = one ? r[t + 3] : r[t + 2];
  }
  if (K >= 2) {
    const bool two = (back & 2) != 0;
    r[t + 0] = two ? r[t + 2] : r[t + 0]; r[t + 1] = two ? r[t + 3] : r[t + 1];
  }
}

// the four widths of a load class, decoded from the register array (every index a compile-time constant: the array stays in registers)
template <int N4, bool kLoZero>
__device__ __forceinline__ uint32_t pipe_range_dispatch(int b, uint32_t (&r)[4 * N4], int back, uint32_t lo, uint32_t span) {
  uint32_t m = 0;
  const uint32_t* words = r;
  switch (b) {
#define PG_CASE(K) case 4 * N4 - K: pipe_align_tail<N4, K>(r, back); range16_private<4 * N4 - K, 0, kLoZero>(words, lo, span, m); range16_private<4 * N4 - K, 1, kLoZero>(words, lo, span, m); break;
    PG_CASE(3) PG_CASE(2) PG_CASE(1) PG_CASE(0)
#undef PG_CASE
    default: break;
  }
  return __builtin_bitreverse32(m);      // value j -> bit j
}

template <int N4>
__device__ __forceinline__ void pipe_agg_dispatch(int b, uint32_t (&r)[4 * N4], int back, uint32_t m, bool need_sum, bool need_minmax,
                                                  uint32_t& psum, unsigned long long& wsum, uint32_t& umin, uint32_t& umax) {
  const uint32_t* words = r;
  switch (b) {
#define PG_CASE(K) case 4 * N4 - K: pipe_align_tail<N4, K>(r, back); agg16_private<4 * N4 - K, 0>(words, m, need_sum, need_minmax, psum, wsum, umin, umax); \
                                    agg16_private<4 * N4 - K, 1>(words, m, need_sum, need_minmax, psum, wsum, umin, umax); break;
    PG_CASE(3) PG_CASE(2) PG_CASE(1) PG_CASE(0)
#undef PG_CASE
    default: break;
  }
}

// backs: the filter chunk's `back` in bits 0-1, the aggregated chunk's in bits 2-3.  One tile from its two chunks in registers: f -> mask, tail mask, popcount; v under the mask.
template <int NF4, int NV4, typename P>
__device__ __forceinline__ void pipe_tile(const P& p, long long tile, int lane, uint32_t (&fw)[4 * NF4], uint32_t (&vw)[4 * NV4], int backs,
                                          unsigned long long& count, unsigned long long& sum, uint32_t& umin, uint32_t& umax) {
  const auto& L = p.nodes[0];
  const auto& ac = p.agg_cols[0];
  uint32_t m = L.lo == 0 ? pipe_range_dispatch<NF4, true>(L.bits, fw, backs, 0u, L.span) : pipe_range_dispatch<NF4, false>(L.bits, fw, backs, (uint32_t)L.lo, L.span);
  if (L.exclusive) m = ~m;
  const long long rem = (long long)p.num_docs - (tile * 2048 + lane * 32);        // docs past numDocs (last tile only)
  m &= rem >= 32 ? 0xFFFFFFFFu : (rem <= 0 ? 0u : ((1u << (int)rem) - 1u));
  count += (unsigned)__builtin_popcount(m);
  uint32_t psum = 0, tmin = 0xFFFFFFFFu, tmax = 0u;
  unsigned long long wsum = 0;
  pipe_agg_dispatch<NV4>(ac.bits, vw, backs >> 2, m, ac.need_sum != 0, ac.need_minmax != 0, psum, wsum, tmin, tmax);
  sum += wsum + psum;
  umin = tmin < umin ? tmin : umin;
  umax = tmax > umax ? tmax : umax;
}

// p.nodes[0]: the range leaf, (bits + 3) / 4 == NF4; p.agg_cols[0]: the aggregated column, (bits + 3) / 4 == NV4 (launch_scan_simple_pipe).
template <int NF4, int NV4, typename P>
__device__ __forceinline__ void scan_simple_pipe_body(const P& p, uint32_t block_index, uint32_t num_blocks, BlockPartial* red, uint32_t* fold_flag_ptr) {
  const int lane = threadIdx.x & 63;
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (uniform: the tile and its bases are scalars)
  const int waves_per_block = blockDim.x >> 6;
  const long long total_waves = (long long)num_blocks * waves_per_block;
  const long long num_tiles = ((long long)p.num_docs + 2047) / 2048;
  const auto& L = p.nodes[0];
  const auto& ac = p.agg_cols[0];
  const GlobalWords f_words = global_words(L.fwd), v_words = global_words(ac.fwd);
  const long long f_tile_words = 64ll * L.bits, v_tile_words = 64ll * ac.bits;
  const int fback = pipe_tail_back<NF4>(lane, L.bits), vback = pipe_tail_back<NV4>(lane, ac.bits);
  const int backs = fback | vback << 2;      // (one register for the two: five waves per SIMD have none to spare)
  const uint32_t f_at = (uint32_t)(lane * L.bits), f_tail = f_at + 4u * (NF4 - 1) - (uint32_t)fback;
  const uint32_t v_at = (uint32_t)(lane * ac.bits), v_tail = v_at + 4u * (NV4 - 1) - (uint32_t)vback;

  unsigned long long count = 0, sum = 0;
  uint32_t umin = 0xFFFFFFFFu, umax = 0u;
  long long tile = (long long)block_index * waves_per_block + wave_in_block;
  if (tile < num_tiles) {
    uint32_t fw[4 * NF4];
    pipe_load_chunk<NF4>(f_words + tile * f_tile_words, f_at, f_tail, fw);
    for (long long next = tile + total_waves; next < num_tiles; next += total_waves) {
      uint32_t vw[4 * NV4], fn[4 * NF4];
      pipe_load_chunk<NV4>(v_words + tile * v_tile_words, v_at, v_tail, vw);
      pipe_load_chunk<NF4>(f_words + next * f_tile_words, f_at, f_tail, fn);
      __builtin_amdgcn_sched_barrier(0);      // the loads stay HERE: the scheduler otherwise sinks v's below the first half of the f decode
      pipe_tile<NF4, NV4>(p, tile, lane, fw, vw, backs, count, sum, umin, umax);
      // f(i+1) becomes f(i).  The copy reads the loaded registers, so the wave waits for f(i+1) here -- behind v(i), which was issued before
      // it and has been waited for and decoded: the wait is short, and the next iteration's f decode waits for nothing.  (Two arrays taking
      // turns over a loop of two steps need no copy and no wait, and nine registers more than five waves per SIMD leave: spilled.)
#pragma unroll
      for (int i = 0; i < 4 * NF4; ++i) fw[i] = fn[i];
      tile = next;
    }
    // The wave's last tile has no next one to request: peeled, so that the loop keeps one shape, no branch in it decides whether a load is
    // issued, and no chunk is read twice.
    uint32_t vw[4 * NV4];
    pipe_load_chunk<NV4>(v_words + tile * v_tile_words, v_at, v_tail, vw);
    __builtin_amdgcn_sched_barrier(0);
    pipe_tile<NF4, NV4>(p, tile, lane, fw, vw, backs, count, sum, umin, umax);
  }

  BlockPartial mine;
  partial_identity(mine);
  mine.count = (unsigned long long)wave_sum_i64((long long)count);
  mine.sum[0] = wave_sum_i64((long long)sum);
  // unsigned keys below 2^31 -> the int32 keys of BlockPartial; lanes that matched nothing keep the identities
  mine.kmin[0] = wave_min_i32(umin == 0xFFFFFFFFu ? 0x7FFFFFFF : (int32_t)umin);
  mine.kmax[0] = wave_max_i32(count == 0ull ? (int32_t)0x80000000 : (int32_t)umax);
  if (lane == 0) red[wave_in_block] = mine;
  __syncthreads();
  publish_block_partial(p, red, waves_per_block, fold_flag_ptr, block_index, num_blocks);
}

// (scan_simple_pipe_kernel<NF4, NV4> itself is defined in pg_unit_scan_simple_pipe.hip)

}  // namespace pg
