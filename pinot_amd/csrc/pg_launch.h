// pg_launch.h -- host-callable launchers of the big kernel templates.  Each family is instantiated in its own translation unit
// (pg_unit_*.hip) so that the four of them compile in parallel; pg_engine.hip only sees these declarations.
#ifndef PG_LAUNCH_H
#define PG_LAUNCH_H
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pg_device.h"

namespace pg {

// Wavefronts per CU the register file admits for a kernel: 512 VGPRs per SIMD lane in 8-register granules, at most 6
// because these kernels use ~100 SGPRs (MI355X_MICROARCH.md: 256-thread blocks admitted = floor(800 / (sgpr granule + 16))).
template <typename K>
int max_waves_per_cu(K kernel) {
  hipFuncAttributes attr;
  if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kernel)) != hipSuccess || attr.numRegs <= 0) return 16;
  const int alloc = ((attr.numRegs + 7) / 8) * 8;
  return std::max(1, std::min(6, 512 / alloc)) * 4;
}
// (kernels with few SGPRs: up to eight waves per SIMD)
template <typename K>
int max_waves_per_cu_lean(K kernel) {
  hipFuncAttributes attr;
  if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kernel)) != hipSuccess || attr.numRegs <= 0) return 16;
  const int alloc = ((attr.numRegs + 7) / 8) * 8;
  return std::max(1, std::min(8, 512 / alloc)) * 4;
}
template <typename K>
void set_dynamic_lds(K kernel, size_t bytes) {
  if (bytes > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// scan_agg_kernel<kDma, slots (1 | kMaxAggCols), typed>: the LDS-staged scan -> filter -> aggregate kernel
void launch_scan_agg(bool dma, bool one_slot, bool typed, int blocks, int threads, size_t lds, hipStream_t stream, const ScanParams& p);
int waves_scan_agg(bool one_slot, bool typed);
// scan_private_kernel<slots>: the lane-private scan -> filter -> aggregate kernel
void launch_scan_private(int agg_cols, int blocks, hipStream_t stream, const ScanParams& p);      // instantiated for 1 and kMaxAggCols slots
int waves_scan_private(int agg_cols);
// scan_private_fsm_kernel<1 | kMaxAggCols>: the same with numEntriesScannedInFilter's transducer walked inside (ScanParams.fsm_*)
void launch_scan_private_fsm(int agg_cols, int blocks, hipStream_t stream, const ScanParams& p);
int waves_scan_private_fsm(int agg_cols);
// scan_private_batch_kernel<slots>: many queries in one launch (pg_execute_batch); items / block_first are device memory
void launch_scan_private_batch(bool one_slot, int total_blocks, hipStream_t stream, const ScanParams* items, const uint32_t* block_first, int num_items);
// scan_sparse_kernel: aggregation of the docs one sparse bitmap names, eight tiles per wave and iteration (pg_scan_sparse.h)
void launch_scan_sparse(bool one_slot, int blocks, hipStream_t stream, const ScanParams& p);      // one_slot: at most one aggregated column
int waves_scan_sparse(bool one_slot);
// scan_simple_kernel: one dictionary-range leaf (or none) + at most one aggregated packed column of <= 20 bits (pg_scan_simple.h)
void launch_scan_simple(int blocks, int threads, hipStream_t stream, const ScanParams& p, bool set_leaf = false);      // threads: kBlockThreads or kWideBlockThreads; set_leaf: scan_simple_set_kernel (the one leaf is a dictId set, looked up in LDS)
int waves_scan_simple();
// scan_simple_pipe_kernel<NF4, NV4>: one dictionary-range leaf AND one aggregated packed column, the two columns' loads pipelined across tiles;
// N = sixteen-byte loads per lane and column (pg_scan_simple_pipe.h).  scan_simple_pipe_shape: the width pair has an instantiation.
bool scan_simple_pipe_shape(int filter_bits, int value_bits);
void launch_scan_simple_pipe(int blocks, int threads, hipStream_t stream, const ScanParams& p);
int waves_scan_simple_pipe();          // the least over the instantiations
// scan_simple_dma_kernel<N, aux>: the pipelined kernel's queries with the two columns streamed through a wave-private ring of kDmaSlots LDS
// slots by LDS-DMA loads (pg_scan_simple_dma.h); every width pair up to kSimpleMaxBits.  nt: the loads are non-temporal (columns read once and
// larger than the Infinity Cache).  Workgroups of kBlockThreads; the dynamic LDS is scan_simple_dma_lds(...).
constexpr int kDmaSlots = 2;      // (three slots leave room for one workgroup per CU at the headline's widths: measured slower)
size_t scan_simple_dma_lds(int filter_bits, int value_bits);
// scan_simple_dma_pair_kernel<FB, VB, aux>: the same ring with both widths compile-time constants, a straight-line tile; one instance per pair
// the rule admits (pg_dma_pairs.h).  scan_simple_dma_pair_shape: the pair has one.  pair: launch it (the generic kernel otherwise).
// Its instances are spread over kDmaPairParts translation units (pg_unit_scan_simple_dma_pair*.hip); part k keeps the table's entries k, k + 3, ...
bool scan_simple_dma_pair_shape(int filter_bits, int value_bits);
typedef void (*DmaKernel)(const ScanParams);
constexpr int kDmaPairParts = 3;
DmaKernel scan_simple_dma_pair_part0(int at, bool nt);
DmaKernel scan_simple_dma_pair_part1(int at, bool nt);
DmaKernel scan_simple_dma_pair_part2(int at, bool nt);
void launch_scan_simple_dma(int blocks, bool nt, bool pair, hipStream_t stream, const ScanParams& p);
int blocks_scan_simple_dma(int filter_bits, int value_bits, size_t lds_budget);      // resident workgroups per CU: registers and LDS
// scan_simple_valid_kernel: the same shape behind one PG_PRED_DOC_SET leaf (p.bitmaps[0] = the doc set; p.nodes[0] = the range leaf, if any);
// skip_empty_tiles: the form whose tiles without a valid doc skip the filter column too
void launch_scan_simple_valid(int blocks, int threads, hipStream_t stream, const ScanParams& p, bool skip_empty_tiles);
int waves_scan_simple_valid();
// scan_raw_kernel: one raw INT range leaf (or no filter) + at most one aggregated raw INT column, five waves per SIMD, coalesced reads (pg_scan_raw.h)
void launch_scan_raw(int blocks, int threads, hipStream_t stream, const ScanParams& p);
int waves_scan_raw();
// scan_raw_set_kernel<4 | 8>: one PG_PRED_RAW_SET leaf (its hash table in `table_bytes` of dynamic LDS) + at most one aggregated raw INT column (pg_scan_raw_set.h)
void launch_scan_raw_set(int key_bytes, int blocks, size_t table_bytes, hipStream_t stream, const ScanParams& p);
int waves_scan_raw_set(int key_bytes);
// raw_set_bitmap_kernel<4 | 8>: the doc-order match bitmap of such a leaf, for every other query shape
void launch_raw_set_bitmap(int key_bytes, int blocks, hipStream_t stream, const RawSetBitmapParams& p);
int waves_raw_set_bitmap(int key_bytes);
// scan_lean_batch_kernel: the shared launch of pg_execute_batch for items of those two shapes (ScanParams.lean_kind), five waves per SIMD
void launch_scan_lean_batch(int kind, int total_blocks, hipStream_t stream, const ScanParams* items, const uint32_t* block_first, int num_items);      // kind: 1 simple, 2 raw (every item)
int waves_scan_lean_batch(int kind);
// scan_narrow_kernel: COUNT(*) / docId bitmap of a filter over columns of at most 8 bits (pg_scan_narrow.h)
void launch_scan_narrow(bool single_leaf, int blocks, hipStream_t stream, const ScanParams& p);      // single_leaf: scan_narrow_single_kernel, eight tiles per iteration
int waves_scan_narrow(bool single_leaf);
// scan_narrow_batch_kernel<single>: pg_execute_batch's shared launch for items of those two shapes
void launch_scan_narrow_batch(bool single_leaf, int total_blocks, hipStream_t stream, const ScanParams* items, const uint32_t* block_first, int num_items);
int waves_scan_narrow_batch(bool single_leaf);
// scan_typed_batch_kernel<slots>: the same for items of scan_private_typed_kernel's shape (agg_slots: the most any item needs -- 1, 2 or kMaxAggCols)
void launch_scan_typed_batch(int agg_slots, int total_blocks, hipStream_t stream, const ScanParams* items, const uint32_t* block_first, int num_items);
int waves_scan_typed_batch(int agg_slots);
// index_and_kernel: the inverted-index children of a root AND, intersected window by window by a persistent grid of one-wave workgroups (pg_index_and.h)
void launch_index_and_kernel(int blocks, hipStream_t stream, const IndexAndParams& ap, uint32_t num_windows);
int waves_index_and();                 // index_and_kernel: wavefronts (= one-wave workgroups, a window in flight each) per CU
int index_and_batch_blocks_per_cu();   // index_and_batch_kernel: workgroups per CU ...
int index_and_batch_block_waves();     // ... of this many independent wavefronts
// index_and_batch_kernel: pg_execute_batch's shared launch for items whose whole device work is index_and_kernel (COUNT(*) over an index-only filter, the gathered aggregation)
void launch_index_and_batch(int total_blocks, hipStream_t stream, const IndexAndParams* items, const uint32_t* block_first, int num_items);
// scan_group_kernel<kDma, kLdsTable>: LDS-staged group-by
void launch_scan_group(bool dma, bool lds_table, int blocks, int threads, size_t lds, hipStream_t stream, const GroupParams& gp);
int waves_scan_group();
// group_private_kernel<kLdsTable>: lane-private group-by (no filter)
void launch_group_private(bool lds_table, int blocks, int threads, size_t lds, hipStream_t stream, const GroupParams& gp);
int waves_group_private();
// group_lds_batch_kernel: pg_execute_batch's shared launch for group-bys of the LDS-table form (items in device memory, one table slice each, `lds` = the largest item's table)
void launch_group_lds_batch(int total_blocks, int threads, size_t lds, hipStream_t stream, const GroupParams* items, const uint32_t* block_first, int num_items);
int waves_group_lds_batch();

// scan_hist_kernel<8 | 16 | 32, guarded>: lane-private scan whose SUM column is counted per dictId in an LDS histogram (pg_scan_hist.h)
void launch_scan_hist(int counter_bits, bool guarded, int blocks, size_t lds, hipStream_t stream, const ScanParams& p);
int waves_scan_hist(int counter_bits, bool guarded);
// scan_hist_batch_kernel<8 | 16 | 32>: pg_execute_batch's shared launch for items of that shape (plain counters; `lds` = the largest item's histogram)
void launch_scan_hist_batch(int counter_bits, int total_blocks, size_t lds, hipStream_t stream, const ScanParams* items, const uint32_t* block_first, int num_items);
int waves_scan_hist_batch(int counter_bits);

// scan_distinct_kernel<lds tier>: DISTINCTCOUNT of up to kMaxAggCols dictionary columns as dictId bitsets, in `lds` bytes of dynamic LDS
// (workgroups of kHistBlockThreads) or straight in HBM (workgroups of 256; `lds`: the filter's set area + the reduction scratch) -- pg_scan_distinct.h
void launch_scan_distinct(bool lds_tier, int blocks, size_t lds, hipStream_t stream, const DistinctParams& dp);
int waves_scan_distinct(bool lds_tier);
// group_distinct_kernel: the same under GROUP BY, one bitset row per raw group id in HBM
void launch_group_distinct(int blocks, size_t lds, hipStream_t stream, const DistinctParams& dp);
int waves_group_distinct();

// scan_counts_kernel<lds tier>: PERCENTILE of up to kMaxAggCols dictionary columns as 32-bit dictId counters, in `lds` bytes of dynamic LDS
// (workgroups of kHistBlockThreads) or straight in HBM (workgroups of 256; `lds`: the filter's set area + the reduction scratch) -- pg_scan_counts.h
void launch_scan_counts(bool lds_tier, int blocks, size_t lds, hipStream_t stream, const DistinctParams& dp);
int waves_scan_counts(bool lds_tier);
// group_counts_kernel: the same under GROUP BY, one counter row per raw group id in HBM
void launch_group_counts(int blocks, size_t lds, hipStream_t stream, const DistinctParams& dp);
int waves_group_counts();

// scan_collect_kernel: PERCENTILE / DISTINCTCOUNT of up to kMaxAggCols raw columns -- the matching docs' order images compacted into one list
// per column (workgroups of 256; `lds`: the filter's set area + the reduction scratch) -- pg_scan_collect.h
void launch_scan_collect(int blocks, size_t lds, hipStream_t stream, const CollectParams& cp);
int waves_scan_collect();
// group_collect_kernel: the same under GROUP BY, every doc's raw group id beside its images
void launch_group_collect(int blocks, size_t lds, hipStream_t stream, const CollectParams& cp);
int waves_group_collect();
// One column's list -> its sorted runs, on `stream`, nothing synchronised: rocPRIM radix sort (GROUP BY: stable by image carrying the row, then
// stable by row over row_bits bits), collect_run_heads_kernel, rocPRIM inclusive scan, collect_run_compact_kernel.
struct CollectSort {
  unsigned long long* images;        // [n] in: the list (spent afterwards)
  unsigned long long* images_work;   // [n] scratch
  const uint32_t* rows;              // [n] in, kept: the docs' raw group ids, or nullptr without GROUP BY
  uint32_t *rows_a, *rows_b;         // [n] each, scratch (GROUP BY)
  int row_bits;                      // bits of the largest raw group id (GROUP BY)
  uint32_t *heads, *position;        // [n] each, scratch
  uint32_t* num_runs;                // [1] out
  void* temp; size_t temp_bytes;     // rocPRIM's scratch: collect_sort_temp_bytes(n) or more
};
struct CollectRuns {                 // where the runs are, device pointers into the scratch above: run j of *num_runs
  unsigned long long* images;        // its order image, ascending (GROUP BY: ascending inside a row)
  uint32_t* first;                   // the list index of its first entry (its count: the next run's first, or n, minus this)
  uint32_t* rows;                    // GROUP BY: its raw group id, ascending
};
hipError_t collect_sort_temp_bytes(size_t n, bool grouped, size_t* out_bytes);
hipError_t collect_sort_runs(const CollectSort& s, size_t n, int num_cus, hipStream_t stream, CollectRuns* out);

// scan_hll_kernel: DISTINCTCOUNTHLL of up to kMaxAggCols raw (column, log2m) slots, their registers in `lds` bytes of dynamic LDS (workgroups of
// kHistBlockThreads), max-merged into the query's rows in HBM -- pg_scan_hll.h
void launch_scan_hll(int blocks, size_t lds, hipStream_t stream, const HllParams& hp);
int waves_scan_hll();
// group_hll_kernel: the same under GROUP BY, one register row per raw group id in HBM (workgroups of 256; `lds`: the filter's set area + the reduction scratch)
void launch_group_hll(int blocks, size_t lds, hipStream_t stream, const HllParams& hp);
int waves_group_hll();
// hll_fold_kernel: `rows` rows of a dictionary column's dictId bitsets -> register rows (chunks / words_per_chunk are set here); rows x chunks workgroups
void launch_hll_fold(long long rows, hipStream_t stream, HllFoldParams fp);
// hll_pack_kernel: n staged 32-bit registers (a multiple of four) -> n bytes
void launch_hll_pack(const uint32_t* words, uint8_t* bytes, unsigned long long n, int num_cus, hipStream_t stream);

// scan_moments_kernel: the pivoted moments {sum(x - c), sum((x - c)^2)} of up to kMaxAggCols raw or dictionary columns, one record per workgroup and
// column (workgroups of 256; `lds`: the filter's set area + the reduction scratch) -- pg_scan_moments.h
void launch_scan_moments(int blocks, size_t lds, hipStream_t stream, const MomentsParams& mp);
int waves_scan_moments();
// group_moments_kernel: the same under GROUP BY, one {S1, S2} row per raw group id in HBM, the pivots read from an uploaded array
void launch_group_moments(int blocks, size_t lds, hipStream_t stream, const MomentsParams& mp);
int waves_group_moments();

// scan_private_typed_kernel: lane-private scan for raw / 8-byte aggregated columns (pg_scan_typed.h)
void launch_scan_private_typed(int agg_cols, int blocks, hipStream_t stream, const ScanParams& p);      // instantiated for 1, 2 and kMaxAggCols slots
int waves_scan_private_typed(int agg_cols);
// partitioned group-by for key spaces above the LDS table (pg_group_partition.h): histogram, scatter, aggregate
void launch_group_partition_histogram(int blocks, hipStream_t stream, const PartitionParams& pp);
void launch_group_partition_scatter(int blocks, hipStream_t stream, const PartitionParams& pp);
void launch_group_partition_aggregate(int work_items, size_t lds, hipStream_t stream, const PartitionParams& pp);
// two-level runs: count / plan / scatter of pass A's records by fine partition (pg_group_partition.h)
void launch_group_repartition(int num_chunks, hipStream_t stream, const RepartitionParams& rp);
void launch_group_typed_direct(int blocks, hipStream_t stream, const GroupParams& gp);   // raw 8-byte aggregation inputs: direct HBM table
int waves_group_partition_scatter();
int blocks_per_cu_group_partition_scatter_packed(int num_partitions);

// chunk_decode_kernel<LZ4 | SNAPPY>: the chunks of a compressed raw forward index -> the dense value area, one wave per chunk, `waves` chunks per
// workgroup in waves * p.lds_stride bytes of dynamic LDS (pg_chunk_decode.h; codec: pgcodec::kLz4 | kSnappy)
struct ChunkDecodeParams;
void launch_chunk_decode(int codec, int blocks, int waves, hipStream_t stream, const ChunkDecodeParams& p);

}  // namespace pg
#endif
