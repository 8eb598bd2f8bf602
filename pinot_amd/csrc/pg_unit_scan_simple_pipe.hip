// Instantiates scan_simple_pipe_kernel<NF4, NV4> -- see pg_launch.h.
#include "pg_scan_simple_pipe.h"
#include "pg_launch.h"

namespace pg {

template <int NF4, int NV4>
__global__ __launch_bounds__(kWideBlockThreads, PG_SIMPLE_WAVES) void scan_simple_pipe_kernel(const ScanParams p) {
  __shared__ BlockPartial red[kWideBlockThreads / 64];      // (launched with kBlockThreads or kWideBlockThreads threads)
  __shared__ uint32_t fold_flag;
  scan_simple_pipe_body<NF4, NV4>(p, blockIdx.x, gridDim.x, red, &fold_flag);
}

typedef void (*PipeKernel)(const ScanParams);
// [NF4 - 1][NV4 - 1].  <4, 5>, <5, 3>, <5, 4> and <5, 5> need one to nine registers more than five waves per SIMD leave: not instantiated,
// scan_simple_pipe_shape declines those pairs and scan_simple_kernel keeps them.
#define K(F, V) scan_simple_pipe_kernel<F, V>
static const PipeKernel kPipeKernels[5][5] = {{K(1, 1), K(1, 2), K(1, 3), K(1, 4), K(1, 5)},
                                              {K(2, 1), K(2, 2), K(2, 3), K(2, 4), K(2, 5)},
                                              {K(3, 1), K(3, 2), K(3, 3), K(3, 4), K(3, 5)},
                                              {K(4, 1), K(4, 2), K(4, 3), K(4, 4), nullptr},
                                              {K(5, 1), K(5, 2), nullptr, nullptr, nullptr}};
#undef K

bool scan_simple_pipe_shape(int filter_bits, int value_bits) {
  if (filter_bits < 1 || filter_bits > kSimpleMaxBits || value_bits < 1 || value_bits > kSimpleMaxBits) return false;
  return kPipeKernels[(filter_bits + 3) / 4 - 1][(value_bits + 3) / 4 - 1] != nullptr;
}

void launch_scan_simple_pipe(int blocks, int threads, hipStream_t stream, const ScanParams& p) {
  const int nf4 = (p.nodes[0].bits + 3) / 4, nv4 = (p.agg_cols[0].bits + 3) / 4;      // (a pair scan_simple_pipe_shape admits: choose_scan_kernel)
  kPipeKernels[nf4 - 1][nv4 - 1]<<<dim3((unsigned)blocks), dim3((unsigned)threads), 0, stream>>>(p);
}

// the least any instantiation admits: one grid rule for the family
int waves_scan_simple_pipe() {
  static const int cap = [] {
    int least = max_waves_per_cu_lean(kPipeKernels[0][0]);
    for (int f = 0; f < 5; ++f) for (int v = 0; v < 5; ++v) if (kPipeKernels[f][v] != nullptr) least = std::min(least, max_waves_per_cu_lean(kPipeKernels[f][v]));
    return least;
  }();
  return cap;
}

}  // namespace pg
