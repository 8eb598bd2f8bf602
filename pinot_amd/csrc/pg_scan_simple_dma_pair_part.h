// The instances of scan_simple_dma_pair_kernel<FB, VB, kAux> (pg_scan_simple_dma.h) of ONE of kDmaPairParts units: the pairs at the places
// PG_DMA_PAIR_PART, PG_DMA_PAIR_PART + kDmaPairParts, ... of pg_dma_pairs.h's table, both cache policies -- generated from that table, so that
// the 204 instances compile as three units side by side.  Included by pg_unit_scan_simple_dma_pair{0,1,2}.hip, which define PG_DMA_PAIR_PART.
#include <utility>

#include "pg_scan_simple_dma.h"
#include "pg_launch.h"

namespace pg {

template <int FB, int VB, int kAux>
__global__ __launch_bounds__(kBlockThreads) void scan_simple_dma_pair_kernel(const ScanParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dma_lds[];      // records, flag and rings: the kernel's only LDS object
  scan_simple_dma_pair_body<FB, VB, kAux>(p, blockIdx.x, gridDim.x, dma_lds);
}

namespace {
constexpr int kPart = PG_DMA_PAIR_PART;
static_assert(kPart >= 0 && kPart < kDmaPairParts, "pg_launch.h declares the parts");
constexpr int kPartPairs = (kDmaPairs - kPart + kDmaPairParts - 1) / kDmaPairParts;
struct PartTable { DmaKernel at[kPartPairs][2]; };
constexpr int part_pair(size_t i) { return dma_pair_at((int)i * kDmaPairParts + kPart); }      // filter bits * 32 + value bits
template <size_t... I>
constexpr PartTable part_table(std::index_sequence<I...>) {
  return PartTable{{{scan_simple_dma_pair_kernel<part_pair(I) / 32, part_pair(I) % 32, 0>, scan_simple_dma_pair_kernel<part_pair(I) / 32, part_pair(I) % 32, 2>}...}};
}
const PartTable kPartTable = part_table(std::make_index_sequence<kPartPairs>());
}  // namespace

#define PG_DMA_PAIR_PART_NAME2(P) scan_simple_dma_pair_part##P
#define PG_DMA_PAIR_PART_NAME(P) PG_DMA_PAIR_PART_NAME2(P)
// `at`: dma_pair_index(filter bits, value bits), at % kDmaPairParts == this part
DmaKernel PG_DMA_PAIR_PART_NAME(PG_DMA_PAIR_PART)(int at, bool nt) { return kPartTable.at[at / kDmaPairParts][nt ? 1 : 0]; }

}  // namespace pg
