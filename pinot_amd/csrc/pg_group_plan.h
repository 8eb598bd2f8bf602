// pg_group_plan.h -- the arithmetic of a group-by's plan: how a key space above the LDS table is cut into partitions,
// when a partition record packs into one dword, when an LDS slot carries count and sum together, how pass B's work is chunked, and where
// everything lies in the partitioned path's record buffer.  Plain host C++, no HIP types.
//
// One source for the readers that must agree: run_group_by's stages and run_partitioned_group_by (pg_engine.hip), the stand-alone check
// (host/check/group_plan_main.cpp) and, through that check's output, the mirror in tests/fuzz_group_cases.py.  The limits themselves
// (kMaxPartitions, kMaxFinePerCoarse, kPartitionChunk, kRepartitionChunk, sizeof(PartitionWork)) stay with the kernels' parameter blocks in
// pg_device.h and come in as arguments.
#pragma once
#include <stdint.h>
#include <stddef.h>

namespace pg {

// A key space of `product` raw keys under `accumulators` distinct (column, SUM|MIN|MAX) pairs.  A partition is 2^shift keys -- as many LDS
// entries of (count dword + one 8-byte slot per accumulator) as pass B's table holds: 4096 up to 20 bytes an entry, else 2048.  More fine
// partitions than one scatter pass addresses: two levels, 2^log2_fine_per_coarse fine partitions per coarse one, pass A scatters by coarse
// partition.
struct PartitionPlan {
  int entry_bytes = 4, shift = 12, log2_fine_per_coarse = 0;
  long long fine_partitions = 0, scatter_partitions = 0;
  bool two_level() const { return log2_fine_per_coarse > 0; }
  int scatter_shift() const { return shift + log2_fine_per_coarse; }      // what pass 0 and pass A shift a raw key by
};
inline PartitionPlan partition_plan(long long product, int accumulators, int max_partitions) {
  PartitionPlan p;
  p.entry_bytes = 4 + 8 * accumulators;
  p.shift = p.entry_bytes <= 20 ? 12 : 11;
  p.fine_partitions = (product + (1ll << p.shift) - 1) >> p.shift;
  while (((p.fine_partitions + (1ll << p.log2_fine_per_coarse) - 1) >> p.log2_fine_per_coarse) > max_partitions) ++p.log2_fine_per_coarse;
  p.scatter_partitions = (p.fine_partitions + (1ll << p.log2_fine_per_coarse) - 1) >> p.log2_fine_per_coarse;
  return p;
}

// One packed dword per doc when the only aggregation input is an unsigned field that fits beside the slot (pg_group_partition.h): the width
// of that field, 1 for COUNT alone, 0 for separate key / value record columns.  `is_sum`, `bits`, `is_raw`, `is_plane`, `is_i32` describe the
// first accumulator (read only when it is the only one); `packing_on` is PINOT_GPU_PARTITION_PACKED.
inline int partition_packed_bits(bool packing_on, int accumulators, bool is_sum, int bits, bool is_raw, bool is_plane, bool is_i32, int scatter_shift) {
  if (!packing_on) return 0;
  if (accumulators == 0) return 1;
  if (accumulators != 1) return 0;
  const bool unsigned_field = !is_raw && is_i32 && (!is_sum || is_plane);
  return unsigned_field && bits + scatter_shift <= 32 ? bits : 0;
}

// Count packing: when a summed value plane is narrow enough, its 64-bit LDS slot carries (count << shift) | sum and the separate count atomic
// disappears.  Safe while a workgroup sees fewer than 2^cbits docs: sum < 2^cbits * 2^bits = 2^shift and count < 2^cbits, so
// cbits + shift <= 64 never carries into or out of the count.
inline int count_bits(long long docs_per_block) {
  int cbits = 1;
  while ((1ll << cbits) <= docs_per_block) ++cbits;
  return cbits;
}
// the shift of a `bits`-wide plane field under that count width; 0: it does not pack
inline int count_packed_shift(int cbits, int bits) { return 2 * cbits + bits <= 64 ? (cbits + bits > 32 ? cbits + bits : 32) : 0; }

// Pass B's chunk: about two rounds of resident workgroups (six per CU) over all `records`, so that the flush of the touched slots (one
// global atomic per slot, accumulator and chunk) stays small next to the records a chunk aggregates; whole 1024s, at least 2^16, at most
// `max_chunk` (kPartitionChunk).
inline uint32_t partition_chunk(unsigned long long records, int num_cus, unsigned long long max_chunk) {
  const unsigned long long per_round = (unsigned long long)num_cus * 6, want = ((records + per_round - 1) / per_round + 1023) & ~1023ull;
  const unsigned long long floor = 1ull << 16, at_least = want > floor ? want : floor;
  return (uint32_t)(at_least < max_chunk ? at_least : max_chunk);
}

// The partitioned path's one device buffer: P scatter partitions over N record slots (the segment's docs rounded up to tiles), every section
// on a 256-byte boundary, in this order:
//   upper[P] | cursor[P] (zeroed together: [0, off_offsets)) | offsets[P + 1] | work[max_work] | key[N] | val[num_vals][N]
// and with two levels behind them
//   key2[N] | val2[num_vals][N] | fine count | fine cursor | work_count (fine_zero_bytes, zeroed together) | fine offsets | work2[max_work2] |
//   chunks[max_chunks]
// `work_bytes` is sizeof(PartitionWork), `repartition_chunk` kRepartitionChunk.
struct PartitionLayout {
  static size_t align(size_t v) { return (v + 255) & ~(size_t)255; }
  bool two_level;
  int num_vals;                                // value record columns: none when the records are packed
  size_t val_stride;                           // bytes from one value column to the next
  size_t fine_slots, max_work, max_work2, max_chunks, fine_zero_bytes;
  size_t off_upper, off_cursor, off_offsets, off_work, off_key, off_val, level1_bytes;
  size_t off_key2, off_val2, off_fine, off_fine_offsets, off_work2, off_chunks, bytes;
  PartitionLayout(int P, size_t N, int num_group_aggs, int packed_bits, int log2_fine_per_coarse, size_t work_bytes, size_t repartition_chunk) {
    two_level = log2_fine_per_coarse > 0;
    num_vals = packed_bits > 0 ? 0 : num_group_aggs;
    val_stride = align(N * 4);
    fine_slots = (size_t)P << log2_fine_per_coarse;
    max_work = N / (1u << 16) + (size_t)P + 1;
    max_work2 = N / (1u << 16) + fine_slots + 1;
    max_chunks = N / repartition_chunk + (size_t)P + 1;
    fine_zero_bytes = 2 * fine_slots * 4 + 64;
    off_upper = 0;
    off_cursor = align(off_upper + (size_t)P * 4);
    off_offsets = align(off_cursor + (size_t)P * 4);
    off_work = align(off_offsets + (size_t)(P + 1) * 4);
    off_key = align(off_work + max_work * work_bytes);
    off_val = align(off_key + N * 4);
    level1_bytes = off_val + (size_t)num_vals * val_stride;
    off_key2 = align(level1_bytes);
    off_val2 = align(off_key2 + N * 4);
    off_fine = align(off_val2 + (size_t)num_vals * val_stride);
    off_fine_offsets = align(off_fine + fine_zero_bytes);
    off_work2 = align(off_fine_offsets + fine_slots * 4);
    off_chunks = align(off_work2 + max_work2 * work_bytes);
    bytes = two_level ? align(off_chunks + max_chunks * work_bytes) : level1_bytes;
  }
};

}  // namespace pg
