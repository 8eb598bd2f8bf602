// Stand-alone check of the ring kernels' pair arithmetic (pg_dma_pairs.h), for a sanitizer build on the CPU (make -C pinot_amd/csrc
// sanitize-dma-pairs): the instance table against the rule, and the compile-time staging of scan_simple_dma_pair_kernel against the run-time
// staging loop of scan_simple_dma_kernel (dma_stage_tile, walked here lane by lane) for all 400 width pairs.
// Exit status 0 and "ok" when every expectation holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../pg_dma_pairs.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using namespace pg;

// dma_stage_tile<N> as the generic kernel runs it: instruction j is the filter's while j < nf; a lane takes part while its sixteen bytes begin
// inside the chunk.  Fills, per instruction, the column (0 / 1), the byte offset in the chunk and the lanes; marks every slot byte written.
struct Piece { int column, at, lanes; };
static std::vector<Piece> stage_tile_at_run_time(int filter_bits, int value_bits, std::vector<int>& slot_writes) {
  const int f_bytes = 256 * filter_bits, v_bytes = 256 * value_bits, nf = (filter_bits + 3) >> 2;
  const int n = (filter_bits + 3) / 4 + (value_bits + 3) / 4;      // (launch_scan_simple_dma)
  std::vector<Piece> out;
  slot_writes.assign((size_t)f_bytes + v_bytes, 0);
  for (int j = 0; j < n; ++j) {
    const bool is_f = j < nf;
    const int at = (is_f ? j : j - nf) * 1024, chunk = is_f ? f_bytes : v_bytes;
    int lanes = 0;
    for (int lane = 0; lane < 64; ++lane) {
      if (at + lane * 16 < chunk) {
        ++lanes;
        const int dst = (is_f ? 0 : f_bytes) + at + lane * 16;
        for (int b = 0; b < 16; ++b) ++slot_writes.at((size_t)dst + b);      // (.at: a write past the slot is a failure of its own)
      }
    }
    out.push_back(Piece{is_f ? 0 : 1, at, lanes});
  }
  return out;
}

int main() {
  // ---- the instance table: the admitted pairs, each once, and nothing else ----
  std::vector<int> seen((size_t)kDmaPairs, 0);
  int admitted = 0;
  for (int f = 0; f <= kDmaMaxBits + 1; ++f)
    for (int v = 0; v <= kDmaMaxBits + 1; ++v) {
      const bool in_rule = f >= 1 && f <= kDmaMaxBits && v >= 1 && v <= kDmaMaxBits && f + v >= 27 && f + v <= 38;
      EXPECT(dma_pair_admitted(f, v) == in_rule);
      const int at = dma_pair_index(f, v);
      if (!in_rule) { EXPECT(at == -1); continue; }
      ++admitted;
      EXPECT(at >= 0 && at < kDmaPairs);
      if (at >= 0 && at < kDmaPairs) {
        ++seen[(size_t)at];
        EXPECT(dma_pair_at(at) == f * 32 + v);      // the table's entry `at` is built for this pair
      }
      // the rule's own terms: the headline's slot at the least, two workgroups' rings in the budget
      EXPECT(dma_slot_bytes(f, v) >= kDmaMinSlotBytes);
      EXPECT(2 * dma_lds_bytes(f, v, kDmaSlotsPerWave, kDmaWavesPerBlock) <= kDmaLdsBudget);
    }
  EXPECT(admitted == kDmaPairs && kDmaPairs == 102);
  for (int at = 0; at < kDmaPairs; ++at) EXPECT(seen[(size_t)at] == 1);
  EXPECT(dma_pair_at(-1) == 0 && dma_pair_at(kDmaPairs) == 0);
  EXPECT(dma_pair_index(10, 17) >= 0 && dma_pair_index(6, 20) == -1 && dma_pair_index(19, 20) == -1 && dma_pair_index(20, 19) == -1 && dma_pair_index(20, 6) == -1);
  EXPECT(dma_slot_bytes(10, 17) == 6912 && dma_lds_bytes(10, 17, 2, 4) == 56320 && dma_lds_bytes(18, 20, 2, 4) == 78848);

  // ---- the staging: compile-time pieces == the run-time loop, for every pair of widths ----
  for (int f = 1; f <= kDmaMaxBits; ++f)
    for (int v = 1; v <= kDmaMaxBits; ++v) {
      std::vector<int> writes;
      const std::vector<Piece> run = stage_tile_at_run_time(f, v, writes);
      EXPECT((int)run.size() == dma_instructions(f, v));
      EXPECT(dma_instructions(f, v) >= 2 && dma_instructions(f, v) <= 10);
      for (const int w : writes) EXPECT(w == 1);      // every byte of the slot exactly once
      size_t j = 0;
      for (int column = 0; column < 2; ++column) {
        const int bits = column == 0 ? f : v;
        EXPECT(dma_pieces(bits) >= 1 && dma_pieces(bits) <= 5);
        for (int piece = 0; piece < dma_pieces(bits) && j < run.size(); ++piece, ++j) {
          // dma_stage_piece: base (0 or 4096) + an immediate of at most 3072, full pieces with 64 lanes, the last with dma_last_lanes
          const int base = piece >= 4 ? 4096 : 0, off = (piece & 3) * 1024;
          EXPECT(off <= 4095);
          EXPECT(run[j].column == column && run[j].at == base + off);
          EXPECT(run[j].lanes == (piece + 1 < dma_pieces(bits) ? 64 : dma_last_lanes(bits)));
        }
        const int last = dma_last_lanes(bits);
        EXPECT(last == 16 || last == 32 || last == 48 || last == 64);
        EXPECT((dma_pieces(bits) - 1) * 1024 + last * 16 == 256 * bits);
      }
      EXPECT(j == run.size());
    }

  if (failures != 0) { fprintf(stderr, "dma_pairs: %d expectation(s) failed\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
