// pg_dma_pairs.h -- the arithmetic of the ring kernels' width pairs (pg_scan_simple_dma.h), in plain C++: the slot and LDS bytes, the LDS-DMA
// instructions of a tile and the lanes of a column's last piece, and which pairs (filter bits, value bits) have an instance of
// scan_simple_dma_pair_kernel -- exactly those plan_scan_simple_dma's rule admits: a slot of at least kDmaMinSlotBytes with room for
// kDmaBlocksPerCu workgroups' rings in the LDS budget.  The launcher (its instance table) and the planner (its rule) both read it from here;
// host/check/dma_pairs_main.cpp holds it against the run-time staging loop's own counts on the CPU (make sanitize-dma-pairs).
#pragma once
#include <cstddef>

namespace pg {

constexpr int kDmaMaxBits = 20;               // the widest column of either side (= kSimpleMaxBits: pg_unit_scan_simple_dma.hip asserts it)
constexpr int kDmaSlotsPerWave = 2;           // (= kDmaSlots of pg_launch.h)
constexpr int kDmaWavesPerBlock = 4;          // (= kBlockThreads / 64)
constexpr int kDmaRecordBytes = 1024;         // the reduction records and the fold flag, in front of the rings
constexpr size_t kDmaLdsBudget = 156 * 1024;  // (= kLdsBudget of pg_engine.hip)
// The rule's figures (DESIGN.md 4.1g has the tables they come from): slots of at least the headline's 6 912 bytes, two workgroups per CU.
constexpr int kDmaMinSlotBytes = 6912;
constexpr int kDmaBlocksPerCu = 2;

// A tile's chunk of a column is 256 * bits bytes, fetched as 1 KiB pieces: 64 lanes x 16 bytes, the last piece with the lanes its remainder needs.
constexpr int dma_pieces(int bits) { return (bits + 3) / 4; }
constexpr int dma_last_lanes(int bits) { return 16 * (bits - 4 * (dma_pieces(bits) - 1)); }      // 16, 32, 48 or 64
constexpr int dma_instructions(int filter_bits, int value_bits) { return dma_pieces(filter_bits) + dma_pieces(value_bits); }      // N
constexpr int dma_slot_bytes(int filter_bits, int value_bits) { return 256 * (filter_bits + value_bits); }
constexpr size_t dma_lds_bytes(int filter_bits, int value_bits, int slots, int waves) {
  return (size_t)kDmaRecordBytes + (size_t)waves * slots * dma_slot_bytes(filter_bits, value_bits);
}

constexpr bool dma_width(int bits) { return bits >= 1 && bits <= kDmaMaxBits; }
// The pairs the rule sends to the ring by itself, and so the pairs with a straight-line instance.
constexpr bool dma_pair_admitted(int filter_bits, int value_bits) {
  return dma_width(filter_bits) && dma_width(value_bits) && dma_slot_bytes(filter_bits, value_bits) >= kDmaMinSlotBytes &&
         kDmaLdsBudget / dma_lds_bytes(filter_bits, value_bits, kDmaSlotsPerWave, kDmaWavesPerBlock) >= (size_t)kDmaBlocksPerCu;
}
// Its place in the instance table: the admitted pairs in (filter bits, value bits) order; -1 for every other pair.
constexpr int dma_pair_index(int filter_bits, int value_bits) {
  if (!dma_pair_admitted(filter_bits, value_bits)) return -1;
  int at = 0;
  for (int f = 1; f <= kDmaMaxBits; ++f)
    for (int v = 1; v <= kDmaMaxBits; ++v) {
      if (f == filter_bits && v == value_bits) return at;
      if (dma_pair_admitted(f, v)) ++at;
    }
  return -1;
}
constexpr int dma_pair_count() {
  int n = 0;
  for (int f = 1; f <= kDmaMaxBits; ++f)
    for (int v = 1; v <= kDmaMaxBits; ++v) n += dma_pair_admitted(f, v) ? 1 : 0;
  return n;
}
constexpr int kDmaPairs = dma_pair_count();
// The pair at `index` of the table, as filter_bits * 32 + value_bits (index in 0 .. kDmaPairs - 1).
constexpr int dma_pair_at(int index) {
  int at = 0;
  for (int f = 1; f <= kDmaMaxBits; ++f)
    for (int v = 1; v <= kDmaMaxBits; ++v)
      if (dma_pair_admitted(f, v) && at++ == index) return f * 32 + v;
  return 0;
}
static_assert(kDmaPairs == 102, "27 <= f + v <= 38, both up to 20 bits");
static_assert(dma_pair_admitted(10, 17) && dma_pair_admitted(7, 20) && dma_pair_admitted(20, 18) && !dma_pair_admitted(6, 20) && !dma_pair_admitted(19, 20), "the rule's edges");

}  // namespace pg
