// Instantiates chunk_decode_kernel<LZ4 | SNAPPY> -- see pg_launch.h.
#include "pg_chunk_decode.h"
#include "pg_launch.h"

namespace pg {

template __global__ void chunk_decode_kernel<pgcodec::kLz4>(const ChunkDecodeParams p);
template __global__ void chunk_decode_kernel<pgcodec::kSnappy>(const ChunkDecodeParams p);

void launch_chunk_decode(int codec, int blocks, int waves, hipStream_t stream, const ChunkDecodeParams& p) {
  const size_t lds = (size_t)waves * p.lds_stride;
  if (codec == pgcodec::kLz4) {
    set_dynamic_lds(chunk_decode_kernel<pgcodec::kLz4>, lds);
    chunk_decode_kernel<pgcodec::kLz4><<<dim3((unsigned)blocks), dim3((unsigned)waves * 64u), lds, stream>>>(p);
  } else {
    set_dynamic_lds(chunk_decode_kernel<pgcodec::kSnappy>, lds);
    chunk_decode_kernel<pgcodec::kSnappy><<<dim3((unsigned)blocks), dim3((unsigned)waves * 64u), lds, stream>>>(p);
  }
}

}  // namespace pg
