// Instantiates scan_simple_dma_kernel<N, kAux> and launches it or an instance of scan_simple_dma_pair_kernel (pg_unit_scan_simple_dma_pair*.hip) -- see pg_launch.h.
#include "pg_scan_simple_dma.h"
#include "pg_launch.h"

namespace pg {

template <int N, int kAux>
__global__ __launch_bounds__(kBlockThreads) void scan_simple_dma_kernel(const ScanParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dma_lds[];      // records, flag and rings: the kernel's only LDS object
  scan_simple_dma_body<N, kDmaSlots, kAux>(p, blockIdx.x, gridDim.x, dma_lds);
}

// [N - 2][nt]: N = 2 .. 10 LDS-DMA instructions per tile (every width pair up to kSimpleMaxBits), aux 0 or 2 (nt)
static_assert((kSimpleMaxBits + 3) / 4 == 5, "N = 2 .. 10");
#define K(N) {scan_simple_dma_kernel<N, 0>, scan_simple_dma_kernel<N, 2>}
static const DmaKernel kDmaKernels[9][2] = {K(2), K(3), K(4), K(5), K(6), K(7), K(8), K(9), K(10)};
#undef K

size_t scan_simple_dma_lds(int filter_bits, int value_bits) { return dma_lds_bytes(filter_bits, value_bits, kDmaSlots, kBlockThreads / 64); }

static_assert(kDmaSlots == kDmaSlotsPerWave, "pg_dma_pairs.h prices the rings this unit launches");

bool scan_simple_dma_pair_shape(int filter_bits, int value_bits) { return dma_pair_index(filter_bits, value_bits) >= 0; }

// The instance of a pair: entry `at` of the table of pg_dma_pairs.h, kept by the unit at % kDmaPairParts.
static DmaKernel dma_pair_kernel(int at, bool nt) {
  static_assert(kDmaPairParts == 3, "one case per unit");
  switch (at % kDmaPairParts) {
    case 0: return scan_simple_dma_pair_part0(at, nt);
    case 1: return scan_simple_dma_pair_part1(at, nt);
    default: return scan_simple_dma_pair_part2(at, nt);
  }
}

void launch_scan_simple_dma(int blocks, bool nt, bool pair, hipStream_t stream, const ScanParams& p) {
  if (pair) {      // (scan_simple_dma_pair_shape(f.bits, v.bits): plan_scan_simple_dma)
    const int at = dma_pair_index(p.nodes[0].bits, p.agg_cols[0].bits);
    const DmaKernel kernel = dma_pair_kernel(at, nt);
    static bool raised[kDmaPairs][2];      // (the attribute is the kernel's: set once, to what its pair needs)
    bool& done = raised[at][nt ? 1 : 0];
    const size_t lds = scan_simple_dma_lds(p.nodes[0].bits, p.agg_cols[0].bits);
    if (!done) { set_dynamic_lds(kernel, lds); done = true; }
    kernel<<<dim3((unsigned)blocks), dim3((unsigned)kBlockThreads), lds, stream>>>(p);
    return;
  }
  const int n = (p.nodes[0].bits + 3) / 4 + (p.agg_cols[0].bits + 3) / 4;      // (widths of 1 .. kSimpleMaxBits: choose_scan_kernel)
  const DmaKernel kernel = kDmaKernels[n - 2][nt ? 1 : 0];
  static bool raised[9][2];      // (the attribute is the kernel's: set once, to what the widest pair needs)
  bool& done = raised[n - 2][nt ? 1 : 0];
  if (!done) { set_dynamic_lds(kernel, scan_simple_dma_lds(kSimpleMaxBits, kSimpleMaxBits)); done = true; }
  kernel<<<dim3((unsigned)blocks), dim3((unsigned)kBlockThreads), scan_simple_dma_lds(p.nodes[0].bits, p.agg_cols[0].bits), stream>>>(p);
}

// Workgroups of kBlockThreads per CU: what the registers admit and what the rings leave of the CU's LDS, whichever is less.  (The registers
// are the generic instances': a pair with an instance has room for two workgroups' rings at the most, two waves per SIMD, which any kernel's
// registers admit.)
int blocks_scan_simple_dma(int filter_bits, int value_bits, size_t lds_budget) {
  static const int reg_waves = [] {
    int least = max_waves_per_cu_lean(kDmaKernels[0][0]);
    for (int n = 0; n < 9; ++n) for (int a = 0; a < 2; ++a) least = std::min(least, max_waves_per_cu_lean(kDmaKernels[n][a]));
    return least;
  }();
  return std::min(reg_waves / (kBlockThreads / 64), (int)(lds_budget / scan_simple_dma_lds(filter_bits, value_bits)));
}

}  // namespace pg
