// Instantiates scan_simple_dma_kernel<N, kAux> -- see pg_launch.h.
#include "pg_scan_simple_dma.h"
#include "pg_launch.h"

namespace pg {

template <int N, int kAux>
__global__ __launch_bounds__(kBlockThreads) void scan_simple_dma_kernel(const ScanParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dma_lds[];      // records, flag and rings: the kernel's only LDS object
  scan_simple_dma_body<N, kDmaSlots, kAux>(p, blockIdx.x, gridDim.x, dma_lds);
}

typedef void (*DmaKernel)(const ScanParams);
// [N - 2][nt]: N = 2 .. 10 LDS-DMA instructions per tile (every width pair up to kSimpleMaxBits), aux 0 or 2 (nt)
static_assert((kSimpleMaxBits + 3) / 4 == 5, "N = 2 .. 10");
#define K(N) {scan_simple_dma_kernel<N, 0>, scan_simple_dma_kernel<N, 2>}
static const DmaKernel kDmaKernels[9][2] = {K(2), K(3), K(4), K(5), K(6), K(7), K(8), K(9), K(10)};
#undef K

size_t scan_simple_dma_lds(int filter_bits, int value_bits) { return dma_lds_bytes(filter_bits, value_bits, kDmaSlots, kBlockThreads / 64); }

void launch_scan_simple_dma(int blocks, bool nt, hipStream_t stream, const ScanParams& p) {
  const int n = (p.nodes[0].bits + 3) / 4 + (p.agg_cols[0].bits + 3) / 4;      // (widths of 1 .. kSimpleMaxBits: choose_scan_kernel)
  const DmaKernel kernel = kDmaKernels[n - 2][nt ? 1 : 0];
  static bool raised[9][2];      // (the attribute is the kernel's: set once, to what the widest pair needs)
  bool& done = raised[n - 2][nt ? 1 : 0];
  if (!done) { set_dynamic_lds(kernel, scan_simple_dma_lds(kSimpleMaxBits, kSimpleMaxBits)); done = true; }
  kernel<<<dim3((unsigned)blocks), dim3((unsigned)kBlockThreads), scan_simple_dma_lds(p.nodes[0].bits, p.agg_cols[0].bits), stream>>>(p);
}

// Workgroups of kBlockThreads per CU: what the registers admit and what the rings leave of the CU's LDS, whichever is less.
int blocks_scan_simple_dma(int filter_bits, int value_bits, size_t lds_budget) {
  static const int reg_waves = [] {
    int least = max_waves_per_cu_lean(kDmaKernels[0][0]);
    for (int n = 0; n < 9; ++n) for (int a = 0; a < 2; ++a) least = std::min(least, max_waves_per_cu_lean(kDmaKernels[n][a]));
    return least;
  }();
  return std::min(reg_waves / (kBlockThreads / 64), (int)(lds_budget / scan_simple_dma_lds(filter_bits, value_bits)));
}

}  // namespace pg
