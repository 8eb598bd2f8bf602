// Stand-alone check of the group-by plan's arithmetic (pg_group_plan.h) with the limits of pg_device.h, for a sanitizer build on the CPU
// (make -C pinot_amd/csrc sanitize-group-plan).  It prints the limits and one `plan` line per (product, accumulators) pair -- what
// tests/test_group_plan_cpu.py compares the Python mirror (tests/fuzz_group_cases.py) with -- and asserts the properties of the partitioned
// path's buffer layout and the edges of the packing and chunk rules.  Exit status 0 and a last line "ok" when every expectation holds.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../pg_device.h"
#include "../../pg_group_plan.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using namespace pg;

struct Section { const char* name; size_t start, bytes; };

static void check_layout(int P, size_t N, int aggs, int packed_bits, int log2_fine) {
  const size_t W = sizeof(PartitionWork);
  const PartitionLayout lay(P, N, aggs, packed_bits, log2_fine, W, kRepartitionChunk);
  const size_t fine_slots = (size_t)P << log2_fine;
  EXPECT(lay.two_level == (log2_fine > 0) && lay.num_vals == (packed_bits > 0 ? 0 : aggs) && lay.fine_slots == fine_slots);
  EXPECT(lay.val_stride % 256 == 0 && lay.val_stride >= N * 4 && lay.val_stride - N * 4 < 256);
  EXPECT(lay.max_work == N / 65536 + (size_t)P + 1 && lay.max_work2 == N / 65536 + fine_slots + 1 && lay.max_chunks == N / kRepartitionChunk + (size_t)P + 1);
  std::vector<Section> s = {{"upper", lay.off_upper, (size_t)P * 4}, {"cursor", lay.off_cursor, (size_t)P * 4}, {"offsets", lay.off_offsets, ((size_t)P + 1) * 4},
                            {"work", lay.off_work, lay.max_work * W}, {"key", lay.off_key, N * 4}};
  for (int a = 0; a < lay.num_vals; ++a) s.push_back({"val", lay.off_val + (size_t)a * lay.val_stride, N * 4});
  if (lay.two_level) {
    s.push_back({"key2", lay.off_key2, N * 4});
    for (int a = 0; a < lay.num_vals; ++a) s.push_back({"val2", lay.off_val2 + (size_t)a * lay.val_stride, N * 4});
    s.push_back({"fine", lay.off_fine, lay.fine_zero_bytes});
    s.push_back({"fine_offsets", lay.off_fine_offsets, fine_slots * 4});
    s.push_back({"work2", lay.off_work2, lay.max_work2 * W});
    s.push_back({"chunks", lay.off_chunks, lay.max_chunks * W});
  }
  // every section on a 256-byte boundary, disjoint, in the documented order; `bytes` covers the last one; nothing wrapped round (the same
  // sum in 128 bits)
  unsigned __int128 wide_end = 0;
  for (size_t i = 0; i < s.size(); ++i) {
    EXPECT(s[i].start % 256 == 0);
    if (i + 1 < s.size()) EXPECT(s[i].start + s[i].bytes <= s[i + 1].start && s[i].start < s[i + 1].start);
    wide_end = ((wide_end + 255) & ~(unsigned __int128)255) + s[i].bytes;
  }
  EXPECT(s.back().start + s.back().bytes <= lay.bytes);
  EXPECT((unsigned __int128)lay.bytes >= wide_end && (unsigned __int128)lay.bytes < wide_end + 256);
  if (!lay.two_level) EXPECT(lay.bytes == lay.level1_bytes);
  EXPECT(lay.off_key2 >= lay.level1_bytes);
  // the first memset [0, off_offsets) is `upper` and `cursor` and their padding, nothing of `offsets`
  EXPECT(lay.off_upper == 0 && lay.off_cursor + (size_t)P * 4 <= lay.off_offsets && lay.off_offsets - (lay.off_cursor + (size_t)P * 4) < 256);
  // the zeroed fine block: count[fine_slots] | cursor[fine_slots] | work_count, ending at or before the fine offsets
  EXPECT(lay.fine_zero_bytes == 2 * fine_slots * 4 + 64 && 2 * fine_slots * 4 + 4 <= lay.fine_zero_bytes && lay.off_fine + lay.fine_zero_bytes <= lay.off_fine_offsets);
}

int main() {
  EXPECT(sizeof(PartitionWork) == 16);
  printf("limits max_partitions %d max_partition_aggs %d max_fine_per_coarse %d repartition_chunk %u partition_chunk %d\n", kMaxPartitions, kMaxPartitionAggs, kMaxFinePerCoarse,
         kRepartitionChunk, kPartitionChunk);
  const long long products[] = {10001, 4096ll * 512 - 1, 4096ll * 512, 4096ll * 512 + 1, 2048ll * 512 - 1, 2048ll * 512, 2048ll * 512 + 1, 1ll << 21, 1ll << 22, 1ll << 23,
                                (1ll << 24) - 1, 1ll << 24, (1ll << 24) + 1, (1ll << 31) - 1};
  for (const long long product : products)
    for (int accumulators = 0; accumulators <= 3; ++accumulators) {
      const PartitionPlan p = partition_plan(product, accumulators, kMaxPartitions);
      printf("plan product %lld accumulators %d entry_bytes %d shift %d fine %lld log2_fine_per_coarse %d scatter %lld\n", product, accumulators, p.entry_bytes, p.shift,
             p.fine_partitions, p.log2_fine_per_coarse, p.scatter_partitions);
      // every key has a fine partition, every fine partition a coarse one, and one scatter pass addresses them all
      EXPECT((p.fine_partitions << p.shift) >= product && ((p.fine_partitions - 1) << p.shift) < product);
      EXPECT((p.scatter_partitions << p.log2_fine_per_coarse) >= p.fine_partitions && p.scatter_partitions >= 1 && p.scatter_partitions <= kMaxPartitions);
      EXPECT(p.log2_fine_per_coarse == 0 || (p.fine_partitions + (1ll << (p.log2_fine_per_coarse - 1)) - 1) >> (p.log2_fine_per_coarse - 1) > kMaxPartitions);
      EXPECT(p.two_level() == (p.fine_partitions > kMaxPartitions) && p.scatter_shift() == p.shift + p.log2_fine_per_coarse);
      EXPECT(((size_t)p.entry_bytes << p.shift) <= 96 * 1024);      // pass B's table fits the LDS
    }
  // 2^31 - 1 keys: kMaxFinePerCoarse fine partitions per coarse one reach them at shift 12; at shift 11 (three accumulators) they reach 2^30
  // keys, and the engine keeps the direct table beyond (choose_group_route)
  EXPECT((1 << partition_plan((1ll << 31) - 1, 2, kMaxPartitions).log2_fine_per_coarse) == kMaxFinePerCoarse);
  EXPECT((1 << partition_plan(1ll << 30, 3, kMaxPartitions).log2_fine_per_coarse) == kMaxFinePerCoarse);
  EXPECT((1 << partition_plan((1ll << 30) + 1, 3, kMaxPartitions).log2_fine_per_coarse) == 2 * kMaxFinePerCoarse);

  const size_t tiles_140000 = ((size_t)140000 + 2047) / 2048 * 2048;
  for (const int P : {1, 2, 511, 512})
    for (const size_t N : {(size_t)2048, (size_t)8192, tiles_140000, (size_t)1 << 31})
      for (int aggs = 0; aggs <= 3; ++aggs)
        for (const int packed_bits : {0, 7})
          for (const int log2_fine : {0, 1, 10}) check_layout(P, N, aggs, packed_bits, log2_fine);

  // packed records: COUNT alone packs one bit; one unsigned field packs while it fits beside the slot; a signed or raw input, a gathered SUM
  // and two accumulators do not; the switch turns all of it off
  EXPECT(partition_packed_bits(true, 0, false, 0, false, false, true, 12) == 1 && partition_packed_bits(false, 0, false, 0, false, false, true, 12) == 0);
  EXPECT(partition_packed_bits(true, 1, true, 20, false, true, true, 12) == 20 && partition_packed_bits(true, 1, true, 21, false, true, true, 12) == 0);
  EXPECT(partition_packed_bits(true, 1, true, 11, false, true, true, 21) == 11 && partition_packed_bits(true, 1, true, 12, false, true, true, 21) == 0);
  EXPECT(partition_packed_bits(true, 1, false, 10, false, false, true, 12) == 10);      // MIN / MAX run on dictIds
  EXPECT(partition_packed_bits(true, 1, true, 10, false, false, true, 12) == 0);        // a SUM that gathers signed dictionary values
  EXPECT(partition_packed_bits(true, 1, false, 10, true, false, true, 12) == 0 && partition_packed_bits(true, 1, true, 10, false, true, false, 12) == 0);
  EXPECT(partition_packed_bits(true, 2, true, 10, false, true, true, 12) == 0 && partition_packed_bits(false, 1, true, 10, false, true, true, 12) == 0);
  // count packing: cbits is the width of docs_per_block; the shift is at least 32; 2 * cbits + bits <= 64 or it does not pack
  EXPECT(count_bits(0) == 1 && count_bits(1) == 1 && count_bits(2) == 2 && count_bits(2047) == 11 && count_bits(2048) == 12 && count_bits((1ll << 31) - 1) == 31 && count_bits(1ll << 31) == 32);
  EXPECT(count_packed_shift(12, 10) == 32 && count_packed_shift(12, 20) == 32 && count_packed_shift(12, 21) == 33 && count_packed_shift(20, 24) == 44);
  EXPECT(count_packed_shift(20, 25) == 0 && count_packed_shift(16, 32) == 48 && count_packed_shift(17, 31) == 0 && count_packed_shift(32, 0) == 32 && count_packed_shift(32, 1) == 0);
  // pass B's chunk: whole 1024s of about records / (6 x CUs), never below 2^16 or above kPartitionChunk
  EXPECT(partition_chunk(0, 256, kPartitionChunk) == 65536 && partition_chunk(65536ull * 1536, 256, kPartitionChunk) == 65536);
  EXPECT(partition_chunk(65536ull * 1536 + 1, 256, kPartitionChunk) == 65536 + 1024 && partition_chunk(1ull << 31, 256, kPartitionChunk) == 1398784);
  EXPECT(partition_chunk(1ull << 32, 256, kPartitionChunk) == (uint32_t)kPartitionChunk && partition_chunk(~0ull >> 1, 1, kPartitionChunk) == (uint32_t)kPartitionChunk);
  if (failures == 0) printf("ok\n");
  return failures == 0 ? 0 : 1;
}
