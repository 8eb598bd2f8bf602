// chunk_decode_kernel<codec>: every chunk of an LZ4- or Snappy-compressed fixed-byte raw forward index decoded into the dense big-endian value
// area a PASS_THROUGH file has (pg_segment_open: the compressed file is uploaded as it is, decoded once, and freed -- afterwards the column
// is an ordinary resident raw column).
//
// What it replaces: ChunkDecompressor.decompress per chunk behind BaseChunkForwardIndexReader.getChunkBuffer (LZ4Decompressor /
// SnappyDecompressor over a direct ByteBuffer), once per chunk and reader context on the CPU plan.
//
// One wave decodes one chunk; a workgroup of W waves takes W chunks at a time and the grid strides over the rest.  The sequence walk is
// wave-uniform: every lane runs the shared parser (pg_chunk_codec.h) over the same token bytes, and the sequence it returns is made scalar
// with readfirstlane.  The copies are wave-parallel, 64 bytes a step: literals from the compressed bytes, a match as
//     out[d + i] = out[d - distance + (i mod distance)]      for i < length, all lanes at once
// which is correct for overlapping matches (distance 1 included) because every source byte lies before d.  The chunk is built in the wave's
// own slice of LDS; each sequence is ordered after the previous one by an LDS fence and a wave barrier (no global store -> load ordering is
// relied on), and a finished chunk goes to HBM in whole dwords, coalesced (16 bytes per lane where the chunk's place allows).  A chunk the
// parser rejects stores nothing and reports (chunk << 8 | error) to the launch's status word with an atomic min: the first bad chunk wins.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_chunk_codec.h"

namespace pg {

struct ChunkDecodeParams {
  const uint8_t* file;            // the compressed file as on disk (device copy, padded by 8 readable bytes)
  unsigned long long file_size;
  unsigned long long header_start;   // of the offset table
  int offset_bytes;               // 4 | 8
  int num_chunks;
  unsigned int chunk_bytes;       // numDocsPerChunk * sizeOfEntry: a full chunk's decoded size and every chunk's stride in `out` (a multiple of 4)
  unsigned int last_chunk_bytes;  // the last chunk's decoded size
  unsigned int lds_stride;        // bytes of LDS per wave: chunk_bytes rounded up to 16
  uint8_t* out;                   // the value area (16-byte aligned)
  unsigned long long* status;     // ~0 before the launch
};

constexpr int kChunkDecodeMaxWaves = 4;      // waves (chunks in flight) per workgroup

__device__ __forceinline__ unsigned long long chunk_file_offset(const ChunkDecodeParams& p, int chunk) {
  const uint8_t* q = p.file + p.header_start + (unsigned long long)chunk * (unsigned long long)p.offset_bytes;
  unsigned long long v = 0;
  for (int i = 0; i < p.offset_bytes; ++i) v = (v << 8) | q[i];
  return v;
}

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// orders the wave's LDS accesses: what the lanes wrote for one sequence is visible to every lane of the wave in the next
__device__ __forceinline__ void lds_sequence_point() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0): every LDS write of this wave has completed
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int CODEC>
__global__ __launch_bounds__(kChunkDecodeMaxWaves * 64) void chunk_decode_kernel(const ChunkDecodeParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t chunk_lds[];
  const int lane = (int)(threadIdx.x & 63);
  const int wave = (int)uniform(threadIdx.x >> 6);
  const int waves = (int)(blockDim.x >> 6);
  uint8_t* out_lds = chunk_lds + (size_t)wave * p.lds_stride;
  for (int chunk = (int)blockIdx.x * waves + wave; chunk < p.num_chunks; chunk += (int)gridDim.x * waves) {
    const unsigned long long begin = chunk_file_offset(p, chunk);
    const unsigned long long end = chunk + 1 < p.num_chunks ? chunk_file_offset(p, chunk + 1) : p.file_size;
    const uint32_t expect = chunk + 1 < p.num_chunks ? p.chunk_bytes : p.last_chunk_bytes;
    const uint8_t* src = p.file + begin;
    pgcodec::Parser parser;
    pgcodec::parser_init(parser, src, (uint32_t)(end - begin), expect);      // (the host validated the table: begin <= end <= file_size, extents below 2^31)
    uint32_t d = 0;
    int result;
    for (;;) {
      pgcodec::Sequence s;
      result = (int)uniform((uint32_t)pgcodec::next_sequence<CODEC>(parser, s));
      if (result != pgcodec::kSeq) break;
      parser.ip = uniform(parser.ip); parser.produced = uniform(parser.produced);
      const uint32_t lit_off = uniform(s.lit_off), lit_len = uniform(s.lit_len), distance = uniform(s.distance), match_len = uniform(s.match_len);
      // the parser guarantees: lit_off + lit_len <= compressed bytes, d + lit_len + match_len <= expect <= lds_stride, 0 < distance <= d + lit_len
      for (uint32_t i = (uint32_t)lane; i < lit_len; i += 64) out_lds[d + i] = src[lit_off + i];
      d += lit_len;
      if (match_len) {
        lds_sequence_point();
        const uint8_t* from = out_lds + (d - distance);
        uint32_t r = (uint32_t)lane % distance;      // (i mod distance), kept incrementally: i advances by 64 a step
        const uint32_t step = 64u % distance;
        for (uint32_t i = (uint32_t)lane; i < match_len; i += 64) {
          out_lds[d + i] = from[r];
          r += step;
          if (r >= distance) r -= distance;
        }
        d += match_len;
      }
      lds_sequence_point();
    }
    if (result != pgcodec::kEnd) {
      if (lane == 0) atomicMin(p.status, ((unsigned long long)chunk << 8) | (unsigned long long)result);
      continue;      // nothing of a rejected chunk reaches HBM
    }
    // expect is a multiple of 4 (sizeOfEntry is 4 or 8); the chunk's place in `out` is a multiple of 4 too, of 16 when chunk_bytes is
    uint8_t* dst = p.out + (unsigned long long)chunk * (unsigned long long)p.chunk_bytes;
    if (((p.chunk_bytes | expect) & 15u) == 0) {
      const uint4* from = reinterpret_cast<const uint4*>(out_lds);
      uint4* to = reinterpret_cast<uint4*>(dst);
      for (uint32_t i = (uint32_t)lane; i < expect / 16; i += 64) to[i] = from[i];
    } else {
      const uint32_t* from = reinterpret_cast<const uint32_t*>(out_lds);
      uint32_t* to = reinterpret_cast<uint32_t*>(dst);
      for (uint32_t i = (uint32_t)lane; i < expect / 4; i += 64) to[i] = from[i];
    }
    lds_sequence_point();      // the stores' LDS reads are done before the next chunk's first write
  }
}

}  // namespace pg
