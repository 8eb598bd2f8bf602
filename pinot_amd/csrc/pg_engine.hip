// pg_engine.hip -- host side of the C ABI declared in include/pinot_gpu.h: HBM-resident segments,
// query lowering to kernel parameter blocks, launches on per-query HIP streams, partial-result readback.
// Everything that computes runs in the kernels of pg_kernels.h; there is no CPU fallback in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <array>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pinot_gpu.h"
#include "pg_device.h"
#include "pg_filter_stats.h"
#include "pg_filter_fsm.h"
#include "pg_fsm_kernels.h"
#include "pg_kernels.h"
#include "pg_launch.h"
#include "pg_rank_image.h"
#include "pg_raw_set_table.h"
#include "pg_hll.h"
#include "pg_set_pass_layout.h"
#include "pg_group_plan.h"
#include "pg_dma_pairs.h"
#include "pg_chunk_decode.h"

namespace {

using namespace pg;

thread_local std::string g_error;

pg_status fail(pg_status st, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
  return st;
}

#define HIP_TRY(expr)                                                                                  \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess)                                                                              \
      return fail(_e == hipErrorOutOfMemory ? PG_ERR_OUT_OF_MEMORY : PG_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, \
                  hipGetErrorString(_e), __FILE__, __LINE__);                                          \
  } while (0)

struct Engine {
  bool initialized = false;
  std::atomic<uint64_t> epoch{0};      // moves with every pg_init: what was lowered under other settings is not reused (pg_segment.plan_cache)
  int device = 0;
  int blocks_per_cu = 0;
  bool raw64_coalesced = true;   // PINOT_GPU_RAW64_COALESCED=0: raw LONG / DOUBLE columns are read lane-contiguously (256 bytes per lane)
  int wide_plane = -1;       // PINOT_GPU_WIDE_PLANE: -1 unfiltered sums of 8-byte dictionaries stream a materialised value column, 0 never, 1 always
  bool partition_stats_cache = true;   // PINOT_GPU_PARTITION_STATS_CACHE=0: run the partition histogram pass in every query
  bool partition_packed = true;   // PINOT_GPU_PARTITION_PACKED=0: always separate key / value record columns
  bool plane_async = true;   // PINOT_GPU_PLANE_ASYNC=0: a query that wants a plane waits for its build
  bool staged_h2d = true;    // PINOT_GPU_STAGED_H2D=0: pg_segment_open copies with plain (pageable) hipMemcpy
  long long exact_stats_docs = 64ll << 20;   // PINOT_GPU_EXACT_FILTER_STATS_DOCS: largest segment whose leap-frogging filters are replayed for numEntriesScannedInFilter
  int flags = 0;
  bool use_dma = true;
  int value_plane = -1;      // -1 auto, 0 never, 1 always (PINOT_GPU_VALUE_PLANE)
  int tile_steps = 0;        // 0 auto, 16 or 32 forced (PINOT_GPU_TILE_STEPS)
  bool double_buffer = false;
  bool direct_result = true; // PINOT_GPU_DIRECT_RESULT=0: the folded partial is copied device -> host with a copy command
  int fold_finalize = -1;    // PINOT_GPU_FOLD_FINALIZE: 1 the scan kernel's last workgroup folds the workgroups' records itself, 0 finalize_partials_kernel
                             // does in a launch of its own, -1 (default) = 1: at every size
  int fold_one_counter = 1;  // PINOT_GPU_FOLD_ONE_COUNTER=0: grids of at most 64 workgroups also arrive on eight shard counters + the top one
  bool poll_result = true;   // PINOT_GPU_POLL_RESULT=0: pg_execute always waits with hipStreamSynchronize instead of spinning on the pinned record's sequence number
  bool distinct_lds = true;  // PINOT_GPU_DISTINCT_LDS=0: DISTINCTCOUNT keeps its dictId bitsets in HBM at every cardinality (scan_distinct_kernel<false>; tests of that tier on small dictionaries)
  bool collect = false;        // PINOT_GPU_COLLECT=1: PERCENTILE / DISTINCTCOUNT on raw columns take the collect pass (pg_scan_collect.h); unset: declined as before, the CPU plan keeps them
  bool chunk_decode_host = false;      // PINOT_GPU_CHUNK_DECODE=host: compressed raw chunks are decoded by the host decoder of pg_chunk_codec.h and uploaded as values (what chunks above PG_CHUNK_DECODE_MAX_BYTES always take)
  bool percentile_lds = true;  // PINOT_GPU_PERCENTILE_LDS=0: PERCENTILE keeps its dictId counters in HBM at every cardinality (scan_counts_kernel<false>; tests of that tier on small dictionaries)
  bool set_lds = true;       // PINOT_GPU_SET_LDS=0: dictId-set leaves (IN lists) of the lane-private scan kernels read their words from memory per doc (rounds 2-6a)
  bool lane_skip = true;     // PINOT_GPU_LANE_SKIP=0: the aggregating kernels load a tile's value bytes for every lane, matches or not
  bool batch_blocks_per_cu_forced = false;
  int batch_blocks_per_cu = 4;    // PINOT_GPU_BATCH_BLOCKS_PER_CU: workgroups per CU a batch launch is cut into (all items together)
  bool scan_raw = true;      // PINOT_GPU_SCAN_RAW=0: raw INT scans stay in scan_private_kernel / scan_private_typed_kernel (four waves per SIMD)
  bool scan_raw_set = true;  // PINOT_GPU_SCAN_RAW_SET=0: a lone IN / NOT IN leaf on a raw column takes the membership pre-pass + the general kernels, like every other shape (pg_scan_raw_set.h)
  int scan_simple_valid = 1;  // PINOT_GPU_SCAN_SIMPLE_VALID=0: `range leaf AND doc set` / the doc set alone stays in the general lane-private kernel; 2: the form of
                             // scan_simple_valid_kernel whose tiles without a valid doc skip the filter column too (pg_scan_simple.h)
  int scan_simple_pipe = 1;   // PINOT_GPU_SCAN_SIMPLE_PIPE: 0 never scan_simple_pipe_kernel, 1 by the estimated selectivity of the leaf (choose_scan_kernel), 2 whenever
                             // the shape allows, whatever the estimate (pg_scan_simple_pipe.h)
  int scan_simple_dma = 1;    // PINOT_GPU_SCAN_SIMPLE_DMA: 0 never scan_simple_dma_kernel, 1 by rule (choose_scan_kernel), 2 whenever the shape allows (pg_scan_simple_dma.h)
  int dma_pair = 1;           // PINOT_GPU_SCAN_SIMPLE_DMA_PAIR: 0 the ring kernel's generic form for every width pair; otherwise scan_simple_dma_pair_kernel where the pair has an instance
  int dma_nt = -1;            // PINOT_GPU_SCAN_SIMPLE_DMA_NT: 0 / 1 forces the default / the non-temporal cache policy; unset = by the columns' size
  int dma_blocks_per_cu = 0;  // PINOT_GPU_SCAN_SIMPLE_DMA_BLOCKS_PER_CU: workgroups per CU (what registers and LDS admit still bounds it); 0 = the rule's
  bool scan_simple = true;   // PINOT_GPU_SCAN_SIMPLE=0: one-leaf / one-column queries stay in scan_private_kernel (half the waves per SIMD)
  bool scan_sparse = true;   // PINOT_GPU_SCAN_SPARSE=0: index-led aggregations scan their listed tiles in scan_private_kernel (one tile per wave and iteration)
  // (read at every pg_init like the rest: they were function-local statics, fixed at their first use in the process, until the kernel
  //  coverage run of round 5 needed both settings in one process)
  bool lean_batch = true;    // PINOT_GPU_LEAN_BATCH=0: items of scan_simple_kernel's shape share the general batch launch
  bool partition_two_level = true;   // PINOT_GPU_PARTITION_TWO_LEVEL=0: key spaces above one scatter pass keep the direct HBM atomics
  bool fsm_perm = true;      // PINOT_GPU_FSM_PERM=0: the transducer pass always walks tables (fsm_tiles_kernel), never byte functions
  int index_and_waves = 0;    // PINOT_GPU_INDEX_AND_WAVES: -k = index_and_kernel's waves take k windows each (grid = windows / k); n > 0 = a persistent grid of n wavefronts per CU; 0 = of as many as are resident
  bool batch_index = true;   // PINOT_GPU_BATCH_INDEX=0: pg_execute_batch runs index-led items (COUNT(*) over an index-only filter, the gathered aggregation) as launches of their own instead of sharing index_and_batch_kernel's
  bool index_gather = true;  // PINOT_GPU_INDEX_GATHER=0: an index-led aggregation always runs scan_sparse_kernel behind index_and_kernel (never inside it)
  bool fsm_fused = true;     // PINOT_GPU_FSM_FUSED=0: the transducer always runs as a pass of its own behind the scan (leaf bitmaps through HBM)
  bool fsm_stats = true;     // PINOT_GPU_FSM_STATS=0: no transducer pass (host replay / upper bound)
  bool fsm_episodes = true;  // PINOT_GPU_FSM_EPISODES=0: a NOT child over a scan leaf stays with the host replay / upper bound (round 4's behaviour)
  bool plan_cache = true;    // PINOT_GPU_PLAN_CACHE=0: pg_execute_batch lowers every item of every call
  bool group_publish = true; // PINOT_GPU_GROUP_PUBLISH=0: the group-by items of a shared launch come back through one copy of all slices and a memset behind the launch
  bool batch_more = true;    // PINOT_GPU_BATCH_MORE=0: items of scan_narrow_kernel's / scan_private_typed_kernel's shape run their own launches
  bool group_one_launch = true;   // PINOT_GPU_GROUP_ONE_LAUNCH=0: pg_execute runs a small group-by as init + kernel + count + scan + compact launches (rounds 1-4)
  bool batch_group = true;   // PINOT_GPU_BATCH_GROUP=0: group-by items run their own launches on a worker thread
  bool batch_hist = true;    // PINOT_GPU_BATCH_HIST=0: items of scan_hist_kernel's shape run their own launch on a worker thread
  bool batch_launch = true;  // PINOT_GPU_BATCH_LAUNCH=0: pg_execute_batch runs every item as a pg_execute of its own on the worker threads (no shared launch)
  bool leap2 = true;         // PINOT_GPU_LEAP2=0: a leap-frogging `a AND b` is not counted on the device (host replay / upper bound instead)
  int sparse_lanes = 32;     // PINOT_GPU_SPARSE_LANES: tiles in which at most this many of the 64 lanes hold a match are aggregated match by match (0 = never)
  bool plane_gcd = true;     // PINOT_GPU_PLANE_GCD=0: planes hold value - min unscaled, never alias the dictId stream
  bool scan_private = true;  // PINOT_GPU_SCAN_PRIVATE=0: always the LDS-staged scan kernel
  bool group_private = true; // PINOT_GPU_GROUP_PRIVATE=0: unfiltered group-by through the LDS-staged kernel
  int group_log_replicas = 3; // PINOT_GPU_GROUP_REPLICAS=0..4: log2 of the most copies of its LDS table group_private_kernel keeps (as many as fit)
  bool group_pack = true;    // PINOT_GPU_GROUP_PACK=0: separate count atomic in the group-by LDS table
  bool scan_typed_private = true;     // PINOT_GPU_SCAN_TYPED_PRIVATE=0: raw / 8-byte aggregated columns stay in the LDS-staged kernel
  bool scan_narrow_single = true;     // PINOT_GPU_SCAN_NARROW_SINGLE=0: a single narrow leaf takes the general narrow kernel (four tiles per iteration)
  bool scan_narrow = true;            // PINOT_GPU_SCAN_NARROW=0: filters over columns of at most 8 bits stay in scan_private_kernel
  bool group_partition = true;        // PINOT_GPU_GROUP_PARTITION=0: key spaces above the LDS table always use direct HBM atomics
  long long partition_min_docs = 1ll << 22;   // ... =force: partition even tiny segments (tests)
  unsigned long long group_table_bytes = 64ull << 30;      // PINOT_GPU_GROUP_TABLE_BYTES: largest direct-indexed group table a query may ask for
  int hist = -1;             // PINOT_GPU_HIST: -1 auto, 0 never, 1 also for arithmetic-progression dictionaries (tests)
  int hist_blocks = 0;       // PINOT_GPU_HIST_BLOCKS: cap on the histogram kernel's workgroups (tests: many docs per counter from a small segment)
  bool hist_guard = false;   // PINOT_GPU_HIST_GUARD=1: start every column in the guarded tier (tests)
  int hist_bits = 0;         // PINOT_GPU_HIST_BITS: 8 / 16 force narrower counters than the cardinality needs (tests of the guard protocol)
  int group_waves = 0;       // PINOT_GPU_GROUP_WAVES: cap on wavefronts per group-by workgroup (default 16)
  int physical_devices = 1;  // hipGetDeviceCount at pg_init
  int logical_devices = 1;   // PINOT_GPU_ALIAS_DEVICES=N (> physical): device ids 0..N-1 are accepted, id d runs on HIP device d mod physical.  Every
                             // per-device structure (batch contexts, deferred launches, placement) is keyed by the LOGICAL id, so a one-GPU box
                             // executes the multi-device paths of pg_execute_batch with N contexts on one chip.
  std::mutex mu;
};
Engine g_engine;
// the HIP device behind a device id of the C ABI (pg_segment_desc.device_id, pg_config.device_id)
// (ids alias only under PINOT_GPU_ALIAS_DEVICES, i.e. when more ids are accepted than devices exist; callers range-check with device_id_ok)
inline int phys_device(int logical) { return (g_engine.logical_devices > g_engine.physical_devices && g_engine.physical_devices > 0) ? logical % g_engine.physical_devices : logical; }
// a device id the C ABI accepts: 0 .. logical_devices - 1 once pg_init has counted them; before pg_init only what HIP itself has
inline bool device_id_ok(int id) {
  if (id < 0) return false;
  if (g_engine.initialized) return id < g_engine.logical_devices;
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess && id < n;
}

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

struct ColumnDev {
  std::string name;
  int stored_type = 0, encoding = 0, bits = 0, cardinality = 0;
  uint8_t* d_fwd_alloc = nullptr;
  uint8_t* d_fwd = nullptr;      // first value byte
  size_t fwd_alloc_bytes = 0;
  int32_t* d_dict = nullptr;
  std::vector<int32_t> h_dict;   // host-order 32-bit values in the kernels' domain: INT values, or (LONG value - value_base)
  // Stored types other than INT.  vkind says how the kernels see the VALUES of the column:
  //   kValI32  INT; or a LONG dictionary whose range fits 31 bits: h_dict / d_dict hold value - value_base ("offset
  //            dictionary"), every 32-bit path (gather, value plane, plane-evaluated ranges) works unchanged and the host adds
  //            count * value_base to the sums;
  //   kValI64  LONG dictionary with a wider range (d_dict64: int64 entries), raw LONG;
  //   kValF64  FLOAT / DOUBLE dictionary (d_dict64: doubles, FLOAT widened exactly), raw DOUBLE;   kValF32  raw FLOAT.
  int vkind = kValI32;
  int64_t value_base = 0;
  std::vector<double> h_dict_f64;       // every dictionary: (double) of the true value (MIN / MAX / group keys / SPI readers)
  std::vector<int64_t> h_dict_i64;      // INT / LONG dictionaries: the true value
  unsigned long long* d_dict64 = nullptr;
  uint8_t* d_inv = nullptr;
  uint64_t inv_size = 0;
  DevContainer* d_dir = nullptr;
  std::vector<DevContainer> h_dir;
  std::vector<int64_t> posting_first;   // [cardinality + 1] index into the container directory
  std::vector<int64_t> posting_docs;    // [cardinality] docs of every posting list (the planner's estimates: summing 15 259 containers per posting on every query was 8 us of host time each)
  unsigned long long* d_null_bitmap = nullptr;   // null value vector expanded to a doc-order bitmap (num_tiles * 32 words), or nullptr
  int nullkey_column = -1;              // nullable dictionary column: index of its hidden null-key image (dictId = cardinality where the doc is null)
  // Raw INT / LONG column as a group key: index of its hidden KEY IMAGE -- the fixed-bit stream of (value - raw_min), cardinality
  // raw_max - raw_min + 1, built the first time the column is grouped by (ensure_key_image).  -1: not a raw INT / LONG column, or its
  // value range does not fit the int dictId domain.  On the image itself: key_image_of = the raw column, key_base = its raw_min.
  int keyimage_column = -1;
  int64_t raw_min = 0, raw_max = -1;    // raw INT / LONG columns: smallest / largest value (one pass at open)
  int key_image_of = -1;
  int64_t key_base = 0;
  int key_image_state = 0;              // 0 placeholder (no stream yet), 2 built; pg_segment::key_image_mu
  // A raw column whose values do not fit the int dictId domain (FLOAT / DOUBLE, INT / LONG over more than 31 bits) gets a RANK image instead
  // (pg_rank_image.h): a dictionary of its distinct values built on the device the first time it is grouped by, and every doc's rank in it.
  // On the image: rank_image = true; cardinality / bits are 0 until it is built; h_rank_keys / d_rank_dict hold the order images of the values.
  bool rank_image = false;
  std::vector<unsigned long long> h_rank_keys;
  unsigned long long* d_rank_dict = nullptr;
  bool borrows_dictionary = false;      // hidden image: d_dict / d_dict64 belong to the column it was made from
  int64_t num_nulls = 0;
  // value plane (built lazily on the device the first time the column is summed)
  uint8_t* d_plane = nullptr;
  int plane_bits = 0;                   // 1..31 packed, 32 = big-endian int32 values
  int64_t plane_base = 0;               // value = plane_base + plane_scale * decoded field (0 / 1 for plane_bits == 32)
  int64_t plane_scale = 1;              // gcd of (value - min): frame of reference + GCD scaling
  bool plane_is_fwd = false;            // arithmetic-progression dictionary: the dictId stream itself is the plane (d_plane == d_fwd)
  int plane_fwd_published = 0;          // 1 once plane_is_fwd and the plane_* fields above are set (release / acquire): such a plane is never built, budgeted or dropped,
                                        // so queries take it without g_planes.mu (64 items of a batch lowered side by side met on that mutex twice each)
  // what the plane of this column would look like (computed once at open: the gcd walks the whole dictionary)
  int64_t shape_base = 0, shape_scale = 1;
  int shape_bits = 0;
  bool shape_is_fwd = false;
  bool plane_ready = false;
  // residency of a materialised plane (g_planes.mu guards all of these): state, queries reading it right now, LRU stamp, bytes
  int plane_state = 0;                  // 0 none, 1 being built on the segment's plane stream, 2 ready
  int plane_users = 0;
  uint64_t plane_last_use = 0;
  size_t plane_bytes = 0;
  hipEvent_t plane_event = nullptr;     // recorded behind the build
  int32_t* d_plane_fields = nullptr;    // scaled dictionary the build kernel reads (freed when the build is seen complete)
  int hist_tier = 0;                    // histogram SUM of this column: 0 plain counters + checksum, 1 guarded counters (a counter once wrapped), 2 not
                                        // used any more (even a guarded counter ran away: the value plane / gather paths serve the column)
};

// Per-query execution context: a stream plus reusable device scratch.  Pooled per segment so that
// concurrent pg_execute calls on one handle never share mutable state.
struct ExecCtx {
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  BlockPartial* d_partials = nullptr;
  int partial_capacity = 0;
  HostRecord* h_record = nullptr;               // pinned and device-mapped: the folding workgroup (or finalize_partials_kernel) writes the result into it
  HostRecord* h_record_dev = nullptr;           // its device-side address
  BlockPartial* h_partial = nullptr;            // = &h_record->partial
  uint32_t* d_done = nullptr;                   // "last block done" arrival counter of the scan kernels (zero between launches)
  unsigned long long seq = 0;                   // sequence number of the context's last launch (HostRecord.seq)
  bool pre_started = false;                     // timed runs: ev[0] has been recorded (some kernel runs before the scan)
  bool pre_enqueued = false;                    // something has been put on the stream ahead of the scan kernel (any run, timed or not)
  // The transducer pass of numEntriesScannedInFilter (pg_filter_fsm.h): the leaves' bitmaps, the tiles' tables, the episode records.  Per
  // CONTEXT since round 6 -- rounds 4-5 kept one scratch per segment under a mutex held across the whole query, so two leap-frogging
  // queries on one segment ran back to back.  h_fsm_stage: pinned, the machine's tables on their way in and the two counts on their way out.
  uint8_t* d_fsm_scratch = nullptr;
  size_t fsm_scratch_bytes = 0;
  uint8_t* h_fsm_stage = nullptr;
  hipEvent_t ev_pass[2] = {nullptr, nullptr};
  int ev_last = 3;                              // timed runs: the event that closes the query's device work (2 when nothing follows the scan kernel)
  std::vector<unsigned long long*> d_bitmaps;   // each num_tiles*32 words
  std::vector<uint32_t*> d_sets;
  std::vector<size_t> set_capacity;
  unsigned long long* d_table = nullptr;
  size_t table_capacity = 0;                    // in 8-byte words
  unsigned long long* h_table = nullptr;        // pinned
  size_t h_table_capacity = 0;
  int32_t* d_gather_in = nullptr;
  uint8_t* d_gather_out = nullptr;
  size_t gather_capacity = 0;
  uint8_t* d_partition = nullptr;               // partitioned group-by: counters, work list and the record buffers
  size_t partition_capacity = 0;
  uint32_t* d_tile_list = nullptr;              // index_and_kernel: surviving 2048-doc tiles (one entry per tile of the segment)
  unsigned long long* d_and_counters = nullptr; // [0] cardinality (u64), [1] low dword: number of listed tiles; [2 ...] index_and_kernel's counter lines (IndexAndParams.shards)
  bool and_counter_dirty = false;               // the counter lines were added to and not yet zeroed again
  unsigned long long* h_and_shards = nullptr;   // pinned: where the lines land
  uint8_t* d_arena = nullptr;                   // DeviceScratch: per-query device scratch (compaction of group-by results)
  size_t arena_capacity = 0, arena_wanted = 0;
  uint8_t* h_groups = nullptr;                  // pinned staging of many-group results
  size_t h_groups_capacity = 0;
  unsigned long long* d_filter_entries = nullptr;   // kNodeCountEntries leaves: numEntriesScannedInFilter counted by the lane-private kernels
  unsigned long long* h_filter_entries = nullptr;   // pinned copy
  uint8_t* d_leap_tables = nullptr;             // kNodeLeapfrog2: one byte per 2048-doc tile (leapfrog2_tile), then one Leap2Summary per 1024 tiles
  Leap2Summary* d_leap_blocks = nullptr;        //   (leapfrog2_chain_tiles_kernel -> leapfrog2_chain_blocks_kernel)
  size_t leap_capacity = 0;
  WindowInfo* d_window_info = nullptr;          // index_and_kernel: {tile mask, matching docs} of every 65 536-doc window
  size_t tile_list_capacity = 0, window_info_capacity = 0;
  uint32_t* d_distinct = nullptr;               // DISTINCTCOUNT: the query's dictId bitsets / bit matrices (pg_scan_distinct.h); PERCENTILE: its dictId counters / counter
                                                // matrices (pg_scan_counts.h) -- one scratch (a query has one or the other), zeroed ahead of every launch
  size_t distinct_capacity = 0;                 // in 32-bit words (part of pg_segment.device_bytes)
};

}  // namespace

// A doc set (pg_doc_set_create): the queryable docIds of an upsert / dedup segment as a dense doc-order bitmap, padded to whole
// 2048-doc tiles like a null bitmap.  The segment's table holds the caller's reference; every lowering that reads the words holds one
// more (Lowered.doc_sets, LoweredItem.doc_sets), so a release never frees a bitmap under a query in flight.
struct DocSet {
  int64_t id = 0;
  unsigned long long* d_words = nullptr;
  uint64_t bytes = 0;
  int64_t cardinality = 0;
  ~DocSet() { if (d_words) (void)hipFree(d_words); }
};

struct pg_segment {
  int device = 0;
  int num_docs = 0;
  int num_tiles = 0;
  int num_cus = 256;
  std::atomic<uint64_t> device_bytes{0};      // (grows after open under three different mutexes -- key images, value planes, the transducer's scratch: atomic, so that no update is lost)
  std::string name;
  std::vector<ColumnDev> cols;          // the caller's columns, then hidden images: key images of raw columns (ColumnDev.keyimage_column), null-key images (nullkey_column)
  int num_user_cols = 0;
  std::mutex key_image_mu;              // building a key image (once per raw column)
  std::mutex ctx_mu;
  // Partitioned group-by: docs per partition of a key-column set, ignoring the filter -- a property of the segment, not of the query.
  // Pass 0 (group_partition_histogram_kernel) computes it the first time a (key columns, shift) combination is grouped by; later
  // queries size their record buffers from the cached counts and skip the pass and its round trip to the host.
  std::mutex partition_stats_mu;
  std::vector<std::pair<std::vector<int>, std::vector<uint32_t>>> partition_stats;      // key = {shift, key columns...}
  hipStream_t plane_stream = nullptr;   // value planes are built here, beside the queries
  uint64_t plane_bytes = 0;             // HBM held by materialised value planes (part of device_bytes)
  std::vector<ExecCtx*> free_ctx;
  std::vector<ExecCtx*> all_ctx;
  // the transducer pass of numEntriesScannedInFilter (device_fsm_filter_stats): leaf bitmaps + tables, one query at a time per segment
  // pg_execute_batch: the last few queries lowered for the shared launch (LoweredItem), so that a server that sends the same query to
  // its segments again and again -- one batch per broker request -- does not lower it again.  plane_epoch moves whenever a value plane of
  // this segment is built or dropped: an item lowered before that reads addresses that may be gone.
  std::atomic<uint64_t> plane_epoch{0};
  std::mutex plan_cache_mu;
  std::vector<std::shared_ptr<const struct LoweredItem>> plan_cache;
  mutable std::mutex doc_sets_mu;
  std::vector<std::shared_ptr<DocSet>> doc_sets;      // the caller's references (pg_doc_set_create .. pg_doc_set_release)
};

// What a query's scan kernel leaves behind for the transducer pass: the bitmap of every input leaf it evaluated itself.

struct FsmSide {
  const pg::fstats::Fsm* fsm = nullptr;
  uint32_t* bitmap[pg::kFsmInputs] = {};        // where input i's doc-order bitmap goes
  bool mapped[pg::kFsmInputs] = {};             // the lowered filter has a LEAF node of its own for input i
  bool kernel_wrote = false;                    // the kernel that ran carries the store (eval_filter_private, no tile list)
  // the rest of the pass's scratch (prepare_fsm_side), for the walk INSIDE the scan kernel (scan_private_fsm_kernel)
  uint32_t* tables = nullptr;                   // [tiles * S] the tiles' tables
  uint32_t* chunks = nullptr;                   // [chunks * S] fsm_chain_kernel's output
  unsigned long long* entries = nullptr;        // fsm_finish_kernel's output
  long long num_tiles = 0, num_chunks = 0;
  bool fused = false;                           // out: the scan kernel walked the transducer itself; its count is in the context's pinned counter
  bool prepared = false;                        // prepare_fsm_side gave it the context's scratch
};
constexpr size_t kAndShardBytes = (size_t)pg::kAndCardinalityShards * 128;      // ExecCtx.d_and_counters + 2 / h_and_shards
constexpr size_t kFsmStageBytes = 64 + (1 + (size_t)fstats::kFsmMaxEpisodeStreams) * ((size_t)pg::kFsmStates << pg::kFsmInputs);      // ExecCtx.h_fsm_stage: the two counts | delta | marks of every episode stream

namespace {

void destroy_ctx(ExecCtx* c) {
  if (!c) return;
  // (round 5: a COUNT(*) over an index-only filter leaves a memset of its counters on the stream BEHIND the answer -- nothing of the context
  //  may be freed under it)
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->h_fsm_stage) (void)hipHostFree(c->h_fsm_stage);
  if (c->d_fsm_scratch) (void)hipFree(c->d_fsm_scratch);
  for (hipEvent_t e : c->ev_pass) if (e) (void)hipEventDestroy(e);
  if (c->d_partials) (void)hipFree(c->d_partials);
  if (c->h_record) (void)hipHostFree(c->h_record);
  if (c->d_done) (void)hipFree(c->d_done);
  for (auto* b : c->d_bitmaps) (void)hipFree(b);
  for (auto* s : c->d_sets) (void)hipFree(s);
  if (c->d_table) (void)hipFree(c->d_table);
  if (c->h_table) (void)hipHostFree(c->h_table);
  if (c->d_gather_in) (void)hipFree(c->d_gather_in);
  if (c->d_gather_out) (void)hipFree(c->d_gather_out);
  if (c->d_partition) (void)hipFree(c->d_partition);
  if (c->d_tile_list) (void)hipFree(c->d_tile_list);
  if (c->d_and_counters) (void)hipFree(c->d_and_counters);
  if (c->h_and_shards) (void)hipHostFree(c->h_and_shards);
  if (c->d_window_info) (void)hipFree(c->d_window_info);
  if (c->d_distinct) (void)hipFree(c->d_distinct);
  if (c->d_arena) (void)hipFree(c->d_arena);
  if (c->h_groups) (void)hipHostFree(c->h_groups);
  if (c->d_filter_entries) (void)hipFree(c->d_filter_entries);
  if (c->d_leap_tables) (void)hipFree(c->d_leap_tables);
  if (c->h_filter_entries) (void)hipHostFree(c->h_filter_entries);
  for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

pg_status acquire_ctx(pg_segment* seg, ExecCtx** out) {
  {
    std::lock_guard<std::mutex> lk(seg->ctx_mu);
    if (!seg->free_ctx.empty()) {
      *out = seg->free_ctx.back();
      seg->free_ctx.pop_back();
      return PG_OK;
    }
  }
  ExecCtx* c = new ExecCtx();
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) for (auto& ev : c->ev) { e = hipEventCreate(&ev); if (e != hipSuccess) break; }
  if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_record, sizeof(HostRecord), hipHostMallocMapped);
  if (e == hipSuccess) { memset(c->h_record, 0, sizeof(HostRecord)); c->h_partial = &c->h_record->partial; }
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&c->h_record_dev, c->h_record, 0);
  if (e == hipSuccess) e = hipMalloc((void**)&c->d_done, 10 * 128);      // fold: eight shards + the top counter; leapfrog2_chain_kernel: one more
  if (e == hipSuccess) e = hipMemsetAsync(c->d_done, 0, 10 * 128, c->stream);      // on the context's OWN stream: ordered before its first kernel (a null-stream memset is not)
  if (e != hipSuccess) {
    destroy_ctx(c);
    return fail(PG_ERR_DEVICE, "creating execution context failed: %s", hipGetErrorString(e));
  }
  {
    std::lock_guard<std::mutex> lk(seg->ctx_mu);
    seg->all_ctx.push_back(c);
  }
  *out = c;
  return PG_OK;
}

void release_ctx(pg_segment* seg, ExecCtx* c) {
  std::lock_guard<std::mutex> lk(seg->ctx_mu);
  seg->free_ctx.push_back(c);
}

struct CtxGuard {
  pg_segment* seg;
  ExecCtx* ctx;
  ~CtxGuard() { if (ctx) release_ctx(seg, ctx); }
};

pg_status ensure_partials(ExecCtx* c, int blocks) {
  if (c->partial_capacity >= blocks + kFoldExtraRecords) return PG_OK;
  if (c->d_partials) (void)hipFree(c->d_partials);
  c->d_partials = nullptr;
  HIP_TRY(hipMalloc((void**)&c->d_partials, sizeof(BlockPartial) * (size_t)(blocks + kFoldExtraRecords)));
  c->partial_capacity = blocks + kFoldExtraRecords;
  return PG_OK;
}

pg_status ensure_bitmap(pg_segment* seg, ExecCtx* c, size_t index) {
  while (c->d_bitmaps.size() <= index) {
    unsigned long long* p = nullptr;
    size_t words = (size_t)std::max(seg->num_tiles, 1) * kMaxTileSteps;
    HIP_TRY(hipMalloc((void**)&p, words * 8));
    c->d_bitmaps.push_back(p);
  }
  return PG_OK;
}

// (the sizes of what the set passes keep in this scratch: pg_set_pass_layout.h)
constexpr size_t kDistinctKeepWords = (size_t)64 << 20;      // a bit matrix above 256 MB is freed after the query instead of staying with the context
pg_status ensure_distinct(pg_segment* seg, ExecCtx* c, size_t words) {
  if (c->distinct_capacity >= words) return PG_OK;
  if (c->d_distinct) { (void)hipFree(c->d_distinct); seg->device_bytes -= c->distinct_capacity * 4; }
  c->d_distinct = nullptr; c->distinct_capacity = 0;
  HIP_TRY(hipMalloc((void**)&c->d_distinct, words * 4));
  c->distinct_capacity = words;
  seg->device_bytes += words * 4;
  return PG_OK;
}
void trim_distinct(pg_segment* seg, ExecCtx* c) {
  if (c->distinct_capacity <= kDistinctKeepWords) return;
  (void)hipFree(c->d_distinct);
  seg->device_bytes -= c->distinct_capacity * 4;
  c->d_distinct = nullptr; c->distinct_capacity = 0;
}

pg_status ensure_set(ExecCtx* c, size_t index, size_t bytes) {
  while (c->d_sets.size() <= index) { c->d_sets.push_back(nullptr); c->set_capacity.push_back(0); }
  if (c->set_capacity[index] < bytes) {
    if (c->d_sets[index]) (void)hipFree(c->d_sets[index]);
    c->d_sets[index] = nullptr;
    size_t cap = std::max<size_t>(bytes, 4096);
    HIP_TRY(hipMalloc((void**)&c->d_sets[index], cap));
    c->set_capacity[index] = cap;
  }
  return PG_OK;
}

constexpr long long kBatchMaxTiles = 32768;       // items of up to 64 Mi docs may share a batch launch (pg_execute_batch); larger ones run their own kernel
constexpr int kMaxGroupSlots = 0x7FFFFFFF;        // raw keys are ints: the reference's ArrayBasedHolder + IntMapBasedHolder range (DictionaryBasedGroupKeyGenerator.java:164-184)
constexpr size_t kGroupTableKeepBytes = 1ull << 31; // a direct-indexed table above this is freed after the query instead of staying with the context
constexpr size_t kArenaKeepBytes = 1ull << 30;      // same for the scratch arena

// hipMalloc'ed scratch of one query, released when it goes out of scope (rare paths only: the hot paths reuse ExecCtx buffers)
// Device scratch of one query, carved out of the context's arena; what does not fit is allocated for the query alone and the arena
// grows before the context's next query, so a steady stream of queries allocates nothing (hipMalloc / hipFree cost ~100 us each and
// synchronise the device: they were most of the host time of a many-group result).
struct DeviceScratch {
  ExecCtx* ctx;
  size_t used = 0, wanted = 0;
  std::vector<void*> overflow;
  explicit DeviceScratch(ExecCtx* c) : ctx(c) {
    if (c->arena_wanted > c->arena_capacity) {
      if (c->d_arena) (void)hipFree(c->d_arena);
      c->d_arena = nullptr; c->arena_capacity = 0;
      const size_t bytes = c->arena_wanted + (c->arena_wanted >> 2);
      if (hipMalloc((void**)&c->d_arena, bytes) == hipSuccess) c->arena_capacity = bytes; else (void)hipGetLastError();
    }
  }
  void* alloc(size_t bytes) {
    const size_t need = (std::max<size_t>(bytes, 8) + 255) & ~(size_t)255;
    wanted += need;
    if (used + need <= ctx->arena_capacity) { void* p = ctx->d_arena + used; used += need; return p; }
    void* p = nullptr;
    if (hipMalloc(&p, need) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    overflow.push_back(p);
    return p;
  }
  ~DeviceScratch() {
    for (void* p : overflow) (void)hipFree(p);
    ctx->arena_wanted = std::max(ctx->arena_wanted, std::min(wanted, kArenaKeepBytes));      // larger requests stay one-off allocations
  }
};

// Pinned host staging of a many-group result (ids, counts, accumulators): the copies off the device run at link speed and the
// conversion into pg_agg_value reads them in place.
pg_status ensure_host_groups(ExecCtx* c, size_t bytes) {
  if (c->h_groups_capacity >= bytes) return PG_OK;
  if (c->h_groups) (void)hipHostFree(c->h_groups);
  c->h_groups = nullptr; c->h_groups_capacity = 0;
  const size_t want = bytes + (bytes >> 2);
  HIP_TRY(hipHostMalloc((void**)&c->h_groups, want, hipHostMallocDefault));
  c->h_groups_capacity = want;
  return PG_OK;
}

pg_status ensure_table(ExecCtx* c, size_t words, size_t host_words) {
  if (c->table_capacity < words) {
    if (c->d_table) (void)hipFree(c->d_table);
    c->d_table = nullptr; c->table_capacity = 0;
    if (hipMalloc((void**)&c->d_table, words * 8) != hipSuccess) {
      (void)hipGetLastError();
      c->d_table = nullptr;
      return fail(PG_ERR_OUT_OF_MEMORY, "group-by table of %zu bytes does not fit the device", words * 8);
    }
    c->table_capacity = words;
  }
  if (c->h_table_capacity < host_words) {
    if (c->h_table) (void)hipHostFree(c->h_table);
    c->h_table = nullptr;
    HIP_TRY(hipHostMalloc((void**)&c->h_table, host_words * 8, hipHostMallocDefault));
    c->h_table_capacity = host_words;
  }
  return PG_OK;
}

// Parse one serialized RoaringBitmap (public RoaringFormatSpec) into container descriptors whose
// offsets are relative to the start of the column's inverted-index buffer.
pg_status parse_roaring(const uint8_t* base, uint64_t start, uint64_t len, std::vector<DevContainer>* out) {
  if (len == 0) return PG_OK;
  if (len < 8) return fail(PG_ERR_INVALID_ARGUMENT, "inverted index: truncated bitmap");
  const uint8_t* data = base + start;
  uint32_t cookie = le32(data);
  uint32_t n;
  const uint8_t* run_flags = nullptr;
  uint64_t pos;
  bool has_run = false;
  if ((cookie & 0xFFFF) == 12347u) {
    has_run = true;
    n = (cookie >> 16) + 1;
    run_flags = data + 4;
    pos = 4 + (n + 7) / 8;
  } else if (cookie == 12346u) {
    n = le32(data + 4);
    pos = 8;
  } else {
    return fail(PG_ERR_INVALID_ARGUMENT, "inverted index: bad roaring cookie %u", cookie);
  }
  const uint8_t* desc = data + pos;
  pos += (uint64_t)n * 4;
  if (!has_run || n >= 4) pos += (uint64_t)n * 4;
  if (pos > len) return fail(PG_ERR_INVALID_ARGUMENT, "inverted index: truncated roaring header");
  for (uint32_t c = 0; c < n; ++c) {
    DevContainer dc;
    dc.key = le16(desc + 4 * c);
    dc.cardinality = le16(desc + 4 * c + 2) + 1;
    dc.num_runs = 0;
    dc.offset = start + pos;
    bool is_run = has_run && ((run_flags[c >> 3] >> (c & 7)) & 1);
    if (is_run) {
      if (pos + 2 > len) return fail(PG_ERR_INVALID_ARGUMENT, "inverted index: truncated run container");
      dc.type = 2;
      dc.num_runs = le16(data + pos);
      pos += 2 + 4ull * dc.num_runs;
    } else if (dc.cardinality > 4096) {
      dc.type = 1;
      pos += 8192;
    } else {
      dc.type = 0;
      pos += 2ull * dc.cardinality;
    }
    if (pos > len) return fail(PG_ERR_INVALID_ARGUMENT, "inverted index: truncated container");
    out->push_back(dc);
  }
  return PG_OK;
}

// ---- host -> HBM at segment open ----
// The caller's index buffers are pageable (mmap-ed segment files): a plain hipMemcpy stages them through one internal bounce buffer on
// one thread (~16-24 GB/s measured on the bench box).  Large buffers instead go through a small pool of pinned bounce buffers, one
// host thread and one stream per slot: each thread copies a 16 MiB chunk into its pinned buffer while its previous chunk is still on
// the wire, so the CPU-side copies of several threads and the DMA overlap and the link is the limit.  One upload at a time.
constexpr size_t kStageChunk = 16u << 20;
constexpr int kStageSlots = 8;
struct StageSlot { hipStream_t stream = nullptr; uint8_t* buf[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr}; };
struct StagePool { std::mutex mu; int device = -1; StageSlot slots[kStageSlots]; };
StagePool g_stage;

void destroy_stage_pool_locked() {
  for (auto& sl : g_stage.slots) {
    for (int b = 0; b < 2; ++b) { if (sl.buf[b]) (void)hipHostFree(sl.buf[b]); if (sl.ev[b]) (void)hipEventDestroy(sl.ev[b]); sl.buf[b] = nullptr; sl.ev[b] = nullptr; }
    if (sl.stream) (void)hipStreamDestroy(sl.stream);
    sl.stream = nullptr;
  }
  g_stage.device = -1;
}

hipError_t h2d_copy(void* dst, const void* src, size_t bytes, int device) {
  if (!g_engine.staged_h2d || bytes < 4 * kStageChunk) return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
  std::lock_guard<std::mutex> lk(g_stage.mu);
  if (g_stage.device != device) {
    destroy_stage_pool_locked();
    for (auto& sl : g_stage.slots) {
      hipError_t e = hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking);
      for (int b = 0; b < 2 && e == hipSuccess; ++b) {
        e = hipHostMalloc((void**)&sl.buf[b], kStageChunk, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.ev[b], hipEventDisableTiming);
      }
      if (e != hipSuccess) { destroy_stage_pool_locked(); (void)hipGetLastError(); return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
    }
    g_stage.device = device;
  }
  const size_t chunks = (bytes + kStageChunk - 1) / kStageChunk;
  std::atomic<size_t> next{0};
  std::atomic<int> error{(int)hipSuccess};
  std::vector<std::thread> workers;
  const int threads = (int)std::min<size_t>(kStageSlots, chunks);
  for (int t = 0; t < threads; ++t) {
    workers.emplace_back([&, t] {
      StageSlot& sl = g_stage.slots[t];
      hipError_t e = hipSetDevice(phys_device(device));
      int b = 0;
      while (e == hipSuccess) {
        const size_t c = next.fetch_add(1);
        if (c >= chunks) break;
        const size_t off = c * kStageChunk, n = std::min(kStageChunk, bytes - off);
        e = hipEventSynchronize(sl.ev[b]);                     // the chunk this buffer carried last has left it (no-op before its first use)
        if (e != hipSuccess) break;
        memcpy(sl.buf[b], (const uint8_t*)src + off, n);
        e = hipMemcpyAsync((uint8_t*)dst + off, sl.buf[b], n, hipMemcpyHostToDevice, sl.stream);
        if (e == hipSuccess) e = hipEventRecord(sl.ev[b], sl.stream);
        b ^= 1;
      }
      const hipError_t done = hipStreamSynchronize(sl.stream);
      if (e == hipSuccess) e = done;
      if (e != hipSuccess) error.store((int)e);
    });
  }
  for (auto& w : workers) w.join();
  return (hipError_t)error.load();
}

void drop_planes_of(pg_segment* seg);

void free_segment(pg_segment* seg) {
  if (!seg) return;
  { std::lock_guard<std::mutex> lk(seg->plan_cache_mu); seg->plan_cache.clear(); }
  { std::lock_guard<std::mutex> lk(seg->doc_sets_mu); seg->doc_sets.clear(); }
  drop_planes_of(seg);
  if (seg->plane_stream) (void)hipStreamDestroy(seg->plane_stream);
  for (auto* c : seg->all_ctx) destroy_ctx(c);
  for (auto& col : seg->cols) {
    if (col.d_fwd_alloc) (void)hipFree(col.d_fwd_alloc);
    if (col.d_dict && !col.borrows_dictionary) (void)hipFree(col.d_dict);
    if (col.d_dict64 && !col.borrows_dictionary) (void)hipFree(col.d_dict64);
    if (col.d_inv) (void)hipFree(col.d_inv);
    if (col.d_dir) (void)hipFree(col.d_dir);
    if (col.d_null_bitmap) (void)hipFree(col.d_null_bitmap);
    if (col.d_rank_dict) (void)hipFree(col.d_rank_dict);
    if (col.plane_event) (void)hipEventDestroy(col.plane_event);
  }
  delete seg;
}

// The key image of raw INT / LONG column `c` (ColumnDev.keyimage_column), built on first use: one pass over the resident column on a
// stream of its own (the queries' streams are non-blocking), under the segment's key-image mutex.  *out_column = the image's index.
pg_status ensure_key_image(pg_segment* seg, int c, int* out_column) {
  ColumnDev& col = seg->cols[(size_t)c];
  if (col.keyimage_column < 0)
    return fail(PG_ERR_UNSUPPORTED, "group-by on raw column %s: only INT / LONG columns whose value range fits an int have a key image", col.name.c_str());
  ColumnDev& image = seg->cols[(size_t)col.keyimage_column];
  if (image.rank_image && __atomic_load_n(&image.key_image_state, __ATOMIC_ACQUIRE) != 2) {
    // the column's own dictionary and the docs' ranks in it: one sort + unique + binary-search pass, once per column and segment
    std::lock_guard<std::mutex> lk(seg->key_image_mu);
    if (image.key_image_state == 3) return fail(PG_ERR_UNSUPPORTED, "group-by on raw column %s: its distinct values do not fit the int dictId domain", col.name.c_str());
    if (image.key_image_state != 2) {
      HIP_TRY(hipSetDevice(phys_device(seg->device)));
      uint8_t* d = nullptr;
      size_t bytes = 0;
      int bits = 0, card = 0;
      const char* why = "";
      const pg_status rst = build_rank_image(col.d_fwd, col.vkind, seg->num_docs, seg->num_tiles, seg->num_cus, &image.d_rank_dict, &image.h_rank_keys, &d, &bytes, &bits, &card, &why);
      if (rst == PG_ERR_UNSUPPORTED) { image.key_image_state = 3; return fail(rst, "group-by on raw column %s: %s", col.name.c_str(), why); }
      if (rst != PG_OK) return fail(rst, "group-by on raw column %s: %s", col.name.c_str(), why);
      image.d_fwd_alloc = d; image.d_fwd = d; image.fwd_alloc_bytes = bytes;
      image.bits = bits; image.cardinality = card;
      seg->device_bytes += bytes + (size_t)card * 8;
      __atomic_store_n(&image.key_image_state, 2, __ATOMIC_RELEASE);
    }
  }
  if (__atomic_load_n(&image.key_image_state, __ATOMIC_ACQUIRE) != 2) {
    std::lock_guard<std::mutex> lk(seg->key_image_mu);
    if (image.key_image_state != 2) {
      const size_t bytes = (size_t)std::max(seg->num_tiles, 1) * 256 * (size_t)image.bits + 64;
      uint8_t* d = nullptr;
      hipStream_t stream = nullptr;
      hipError_t e = hipMalloc((void**)&d, bytes);
      if (e != hipSuccess) return fail(PG_ERR_OUT_OF_MEMORY, "key image of column %s: hipMalloc(%zu): %s", col.name.c_str(), bytes, hipGetErrorString(e));
      e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
      if (e == hipSuccess) e = hipMemsetAsync(d, 0, bytes, stream);
      if (e == hipSuccess) {
        build_raw_key_image_kernel<<<dim3((unsigned)std::max(1, std::min(seg->num_tiles / 4 + 1, seg->num_cus * 8))), dim3(256), 0, stream>>>(col.d_fwd, col.vkind == kValI32 ? 4 : 8, image.key_base, d,
                                                                                                                                               image.bits, seg->num_tiles, seg->num_docs);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      if (stream) (void)hipStreamDestroy(stream);
      if (e != hipSuccess) { (void)hipFree(d); return fail(PG_ERR_DEVICE, "key image of column %s: %s", col.name.c_str(), hipGetErrorString(e)); }
      image.d_fwd_alloc = d; image.d_fwd = d; image.fwd_alloc_bytes = bytes;
      seg->device_bytes += bytes;
      __atomic_store_n(&image.key_image_state, 2, __ATOMIC_RELEASE);
    }
  }
  if (out_column) *out_column = col.keyimage_column;
  return PG_OK;
}

// ---- value planes ----
// Policy: summing a dictionary column through its dictionary costs one L2 gather per matching row; a gather costs the
// L2 as much as streaming ~22 bytes, so unless the dictionary is tiny (L1-resident) or the plane would be much wider
// than the dictId stream, the plane wins as soon as a few percent of the rows match.
// Frame of reference + GCD: field = (value - min) / g with g = gcd of all (value - min); w = bits of the largest field.
// When the dictionary is an arithmetic progression (field[d] == d: dense ids, fixed-step values) the dictId stream already IS
// the plane and nothing is materialised.  PINOT_GPU_PLANE_GCD=0 keeps g = 1.
struct PlaneShape { int64_t base; int64_t scale; int bits; bool is_fwd; };
PlaneShape plane_shape(const ColumnDev& col) { return PlaneShape{col.shape_base, col.shape_scale, col.shape_bits, col.shape_is_fwd}; }
PlaneShape compute_plane_shape(const ColumnDev& col) {
  PlaneShape ps;
  const int64_t lo = col.h_dict.front(), hi = col.h_dict.back();
  int64_t g = 0;
  if (g_engine.plane_gcd) {
    for (size_t d = 1; d < col.h_dict.size() && g != 1; ++d) {
      int64_t a = (int64_t)col.h_dict[d] - lo, b = g;
      while (b) { const int64_t t = a % b; a = b; b = t; }
      g = a;
    }
  }
  if (g <= 0) g = 1;
  const int64_t top = (hi - lo) / g;
  int w = 1;
  while (w < 32 && (top >> w) != 0) ++w;
  ps.base = w == 32 ? 0 : lo;
  ps.scale = w == 32 ? 1 : g;
  ps.bits = w;
  ps.is_fwd = g_engine.plane_gcd && w < 32 && top == (int64_t)col.h_dict.size() - 1;     // sorted distinct multiples: field[d] == d
  if (ps.is_fwd) ps.bits = col.bits;
  return ps;
}

bool want_value_plane(const ColumnDev& col) {
  if (col.encoding != PG_FWD_FIXED_BIT_DICT || col.cardinality < 1 || col.vkind != kValI32) return false;
  if (g_engine.value_plane == 0) return false;
  if (g_engine.value_plane == 1) return true;
  const PlaneShape ps = plane_shape(col);
  return ps.is_fwd || col.cardinality > 8192 || ps.bits - col.bits <= 8;
}

// Wide plane: SUM over a LONG / FLOAT / DOUBLE dictionary is one 8-byte L2 gather per doc (2.5e11 /s: 6.6 % of the HBM roofline on an
// unfiltered 250 M-row column).  Materialising the values once -- plane[doc] = dictionary[dictId[doc]], big-endian like a raw column --
// turns the column into a raw 8-byte stream that scan_private_typed_kernel reads with 16-byte loads.  Worth its 8 bytes per doc of
// traffic when most docs match: taken when the query has no filter (PINOT_GPU_WIDE_PLANE=1: always, =0: never) and sums the column
// without taking its MIN / MAX (those run on dictIds); aggregation-only queries.
bool want_wide_plane(const pg_segment* seg, const pg_query* q, int column) {
  if (g_engine.wide_plane == 0 || q->num_group_by > 0 || column < 0 || column >= (int)seg->cols.size()) return false;
  const ColumnDev& col = seg->cols[(size_t)column];
  if (col.encoding != PG_FWD_FIXED_BIT_DICT || col.cardinality < 1 || (col.vkind != kValI64 && col.vkind != kValF64)) return false;
  if (g_engine.wide_plane != 1 && q->num_filter_nodes > 0) return false;
  bool summed = false;
  for (int a = 0; a < q->num_aggregations; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    if (ag.column != column) continue;
    if (ag.function == PG_AGG_MIN || ag.function == PG_AGG_MAX) return false;
    summed |= ag.function == PG_AGG_SUM || ag.function == PG_AGG_AVG;
  }
  return summed;
}

// ---- histogram SUM (pg_scan_hist.h) ----
// SUM(col) = sum_d matches[d] * dictionary[d]: the kernel counts the matching docs per dictId in LDS and never reads a value per
// row.  It reads exactly the dictId stream, so it is preferred over a value plane whenever the histogram fits the CU's LDS --
// except for arithmetic-progression dictionaries, whose dictId stream already is the plane (same bytes, fewer VALU ops per doc).
constexpr size_t kHistLdsBytes = 152 * 1024;      // of 160 KiB: the rest holds the workgroup's reduction records
int hist_counter_bits(const ColumnDev& col) {
  const size_t C = (size_t)std::max(col.cardinality, 1);
  int cw = C * 4 <= kHistLdsBytes ? 32 : (C * 2 <= kHistLdsBytes ? 16 : (C <= kHistLdsBytes ? 8 : 0));
  if (cw > 0 && g_engine.hist_bits > 0) cw = std::min(cw, g_engine.hist_bits);
  return cw;
}
bool want_hist(const ColumnDev& col) {
  if (col.encoding != PG_FWD_FIXED_BIT_DICT || col.cardinality < 1 || col.vkind != kValI32 || col.bits > 18) return false;
  if (g_engine.hist == 0 || __atomic_load_n(&col.hist_tier, __ATOMIC_RELAXED) >= 2) return false;
  if (hist_counter_bits(col) == 0) return false;
  return g_engine.hist == 1 || !plane_shape(col).is_fwd;
}

// ---- value-plane residency ----
// A materialised plane costs about as much HBM as the column itself, so planes live under a budget (pg_config.plane_budget_bytes,
// PINOT_GPU_PLANE_BUDGET_BYTES, pg_set_plane_budget) shared by all segments of the process: a plane is built the first time its
// column is summed, on the segment's own plane stream -- the query that asked does not wait for it, it runs the path that reads the
// dictionary instead (same result), and so does every query until the build is seen complete -- and when the budget is exceeded the
// least recently used planes nobody is reading are released first.  PINOT_GPU_PLANE_ASYNC=0 builds in line (the query waits).
struct PlaneRegistry {
  std::mutex mu;
  std::vector<std::pair<pg_segment*, int>> resident;      // planes in state 1 or 2
  uint64_t total_bytes = 0;
  uint64_t budget_bytes = ~0ull;
  uint64_t tick = 0;
};
PlaneRegistry g_planes;

// g_planes.mu held.  Frees the plane of (seg, column); it must be ready and unused.
void drop_plane_locked(pg_segment* seg, int column) {
  ColumnDev& col = seg->cols[(size_t)column];
  if (col.d_plane && !col.plane_is_fwd) (void)hipFree(col.d_plane);
  col.d_plane = nullptr;
  col.plane_ready = false;
  col.plane_state = 0;
  __atomic_store_n(&col.plane_fwd_published, 0, __ATOMIC_RELEASE);      // (only a closing segment drops a plane that aliases its forward index)
  g_planes.total_bytes -= col.plane_bytes;
  seg->plane_bytes -= col.plane_bytes;
  seg->device_bytes -= col.plane_bytes;
  col.plane_bytes = 0;
  seg->plane_epoch.fetch_add(1, std::memory_order_release);
  auto& r = g_planes.resident;
  r.erase(std::remove(r.begin(), r.end(), std::make_pair(seg, column)), r.end());
}

// Every plane of a segment that is going away (no query is running on it any more).
void drop_planes_of(pg_segment* seg) {
  std::lock_guard<std::mutex> lk(g_planes.mu);
  for (int c = 0; c < (int)seg->cols.size(); ++c) {
    ColumnDev& col = seg->cols[(size_t)c];
    if (col.plane_state == 0) continue;
    if (col.plane_event) (void)hipEventSynchronize(col.plane_event);
    if (col.d_plane_fields) { (void)hipFree(col.d_plane_fields); col.d_plane_fields = nullptr; }
    drop_plane_locked(seg, c);
  }
}

// Asks for the value plane of a column.  *ready: the plane can be read by this query (release_plane when the query is over);
// otherwise the query runs without it.  Never blocks on a build unless PINOT_GPU_PLANE_ASYNC=0.
pg_status acquire_plane(pg_segment* seg, int column, bool* ready) {
  *ready = false;
  ColumnDev& col = seg->cols[(size_t)column];
  if (__atomic_load_n(&col.plane_fwd_published, __ATOMIC_ACQUIRE) != 0) { *ready = true; return PG_OK; }
  std::lock_guard<std::mutex> lk(g_planes.mu);
  if (col.plane_state == 0 && col.vkind != kValI32) {
    // wide plane (want_wide_plane): 8 bytes per doc, padded to whole 2048-doc tiles like a raw column
    const size_t bytes = (size_t)std::max(seg->num_tiles, 1) * 2048 * 8 + 64;
    while (g_planes.total_bytes + bytes > g_planes.budget_bytes) {
      int best = -1;
      for (int i = 0; i < (int)g_planes.resident.size(); ++i) {
        const ColumnDev& c = g_planes.resident[(size_t)i].first->cols[(size_t)g_planes.resident[(size_t)i].second];
        if (c.plane_state != 2 || c.plane_users != 0 || c.plane_is_fwd) continue;
        if (best < 0 || c.plane_last_use < g_planes.resident[(size_t)best].first->cols[(size_t)g_planes.resident[(size_t)best].second].plane_last_use) best = i;
      }
      if (best < 0) return PG_OK;
      drop_plane_locked(g_planes.resident[(size_t)best].first, g_planes.resident[(size_t)best].second);
    }
    HIP_TRY(hipSetDevice(phys_device(seg->device)));
    if (!seg->plane_stream) HIP_TRY(hipStreamCreateWithFlags(&seg->plane_stream, hipStreamNonBlocking));
    if (!col.plane_event) HIP_TRY(hipEventCreateWithFlags(&col.plane_event, hipEventDisableTiming));
    uint8_t* plane = nullptr;
    if (hipMalloc((void**)&plane, bytes) != hipSuccess) { (void)hipGetLastError(); return PG_OK; }
    HIP_TRY(hipMemsetAsync(plane, 0, bytes, seg->plane_stream));
    materialize_wide_plane_kernel<<<dim3((unsigned)std::max(1, seg->num_cus * 8)), dim3(256), 0, seg->plane_stream>>>(col.d_fwd, col.bits, col.d_dict64,
                                                                                                                       reinterpret_cast<unsigned long long*>(plane), seg->num_docs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(col.plane_event, seg->plane_stream));
    col.d_plane = plane;
    col.plane_bytes = bytes;
    col.plane_state = 1;
    g_planes.total_bytes += bytes;
    seg->plane_bytes += bytes;
    seg->device_bytes += bytes;
    g_planes.resident.emplace_back(seg, column);
    seg->plane_epoch.fetch_add(1, std::memory_order_release);
  }
  if (col.plane_state == 0) {
    const PlaneShape ps = plane_shape(col);
    col.plane_bits = ps.bits;
    col.plane_base = ps.base;
    col.plane_scale = ps.scale;
    if (ps.is_fwd) {                       // arithmetic-progression dictionary: the dictId stream is the plane, nothing to build or to budget
      col.plane_is_fwd = true;
      col.d_plane = col.d_fwd;
      col.plane_ready = true;
      col.plane_state = 2;
      __atomic_store_n(&col.plane_fwd_published, 1, __ATOMIC_RELEASE);
      seg->plane_epoch.fetch_add(1, std::memory_order_release);
      *ready = true;
      return PG_OK;
    }
    const int w = ps.bits;
    const size_t bytes = (size_t)std::max(seg->num_tiles, 1) * 256 * (size_t)w + 64;
    // make room: least recently used first, only planes nobody reads
    while (g_planes.total_bytes + bytes > g_planes.budget_bytes) {
      int best = -1;
      for (int i = 0; i < (int)g_planes.resident.size(); ++i) {
        const ColumnDev& c = g_planes.resident[(size_t)i].first->cols[(size_t)g_planes.resident[(size_t)i].second];
        if (c.plane_state != 2 || c.plane_users != 0 || c.plane_is_fwd) continue;
        if (best < 0 || c.plane_last_use < g_planes.resident[(size_t)best].first->cols[(size_t)g_planes.resident[(size_t)best].second].plane_last_use) best = i;
      }
      if (best < 0) return PG_OK;          // nothing can go: this column is served without a plane
      drop_plane_locked(g_planes.resident[(size_t)best].first, g_planes.resident[(size_t)best].second);
    }
    HIP_TRY(hipSetDevice(phys_device(seg->device)));
    if (!seg->plane_stream) HIP_TRY(hipStreamCreateWithFlags(&seg->plane_stream, hipStreamNonBlocking));
    if (!col.plane_event) HIP_TRY(hipEventCreateWithFlags(&col.plane_event, hipEventDisableTiming));
    uint8_t* plane = nullptr;
    if (hipMalloc((void**)&plane, bytes) != hipSuccess) { (void)hipGetLastError(); return PG_OK; }      // no room on the device either: no plane
    HIP_TRY(hipMemsetAsync(plane, 0, bytes, seg->plane_stream));
    // the kernel writes dict'[dictId] where dict' = the scaled fields (for scale 1: value - base through the base argument)
    if (ps.scale != 1) {
      std::vector<int32_t> fields(col.h_dict.size());
      for (size_t d = 0; d < fields.size(); ++d) fields[d] = (int32_t)(((int64_t)col.h_dict[d] - ps.base) / ps.scale);
      HIP_TRY(hipMalloc((void**)&col.d_plane_fields, fields.size() * 4));
      HIP_TRY(hipMemcpy(col.d_plane_fields, fields.data(), fields.size() * 4, hipMemcpyHostToDevice));
    }
    DevColumn dc;
    memset(&dc, 0, sizeof(dc));
    dc.fwd = col.d_fwd; dc.dict = col.d_plane_fields ? col.d_plane_fields : col.d_dict; dc.bits = col.bits; dc.cardinality = col.cardinality; dc.dict_bytes = col.cardinality * 4;
    const int in_slot = ((256 * col.bits + 16) + 15) & ~15;
    const int waves = 4;
    const size_t lds = (size_t)waves * (size_t)(in_slot + 64 * w * 4 + 16);
    const int blocks = (int)std::max<long long>(1, std::min<long long>(((long long)seg->num_tiles + waves - 1) / waves, (long long)seg->num_cus * 2));
    set_dynamic_lds(materialize_plane_kernel, lds);
    materialize_plane_kernel<<<dim3((unsigned)blocks), dim3(waves * 64), lds, seg->plane_stream>>>(dc, plane, w, col.d_plane_fields ? 0 : (int32_t)col.plane_base, seg->num_docs,
                                                                                                    seg->num_tiles, in_slot);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(col.plane_event, seg->plane_stream));
    col.d_plane = plane;
    col.plane_bytes = bytes;
    col.plane_state = 1;
    g_planes.total_bytes += bytes;
    seg->plane_bytes += bytes;
    seg->device_bytes += bytes;
    g_planes.resident.emplace_back(seg, column);
    seg->plane_epoch.fetch_add(1, std::memory_order_release);
  }
  if (col.plane_state == 1) {
    const hipError_t built = g_engine.plane_async ? hipEventQuery(col.plane_event) : hipEventSynchronize(col.plane_event);
    if (built == hipErrorNotReady) return PG_OK;
    if (built != hipSuccess) return fail(PG_ERR_DEVICE, "value plane of %s: %s", col.name.c_str(), hipGetErrorString(built));
    if (col.d_plane_fields) { (void)hipFree(col.d_plane_fields); col.d_plane_fields = nullptr; }
    col.plane_ready = true;
    col.plane_state = 2;
    seg->plane_epoch.fetch_add(1, std::memory_order_release);
  }
  col.plane_users++;
  col.plane_last_use = ++g_planes.tick;
  *ready = true;
  return PG_OK;
}

void release_plane(pg_segment* seg, int column) {
  ColumnDev& col = seg->cols[(size_t)column];
  if (__atomic_load_n(&col.plane_fwd_published, __ATOMIC_ACQUIRE) != 0) return;      // (never counted: acquire_plane)
  std::lock_guard<std::mutex> lk(g_planes.mu);
  if (col.plane_users > 0) col.plane_users--;
}

// The planes a query holds, released on every way out of execute_impl.
struct PlaneHold {
  pg_segment* seg;
  std::vector<int> columns;
  PlaneHold(pg_segment* s, std::vector<int> c) : seg(s), columns(std::move(c)) {}
  PlaneHold(const PlaneHold&) = delete;
  PlaneHold& operator=(const PlaneHold&) = delete;
  PlaneHold(PlaneHold&& o) noexcept : seg(o.seg), columns(std::move(o.columns)) { o.columns.clear(); }
  ~PlaneHold() { for (int c : columns) release_plane(seg, c); }
};

// ---- query lowering ----
struct Lowered {
  PlanParams plan;                    // host-side plan (columns, leaves, nodes) ...
  ScanParams sp;                      // ... flattened into the kernel parameter block by flatten_plan()
  std::vector<int> col_of_slot;       // segment column index * 2 + (1 if the slot streams the value plane)
  std::vector<char> plane_cols;       // per segment column: aggregations read it through its value plane
  int num_scan_leaves = 0;
  int max_bits = 1;
  // index_and_kernel ran for the inverted-index children of the root AND: every match lies in one of the listed tiles
  const uint32_t* tile_list = nullptr;
  const uint32_t* tile_count = nullptr;
  const unsigned long long* d_cardinality = nullptr;
  bool index_and_is_whole_filter = false;      // the filter is exactly that AND: its cardinality answers COUNT(*)
  // ... and its bitmap is stored sparsely (tiles without a match are not written): a reader that does not go by the tile list calls
  // complete_index_and_bitmap first
  unsigned long long* and_bitmap = nullptr;
  const WindowInfo* and_info = nullptr;
  long long and_words = 0;
  // numEntriesScannedInFilter: how this query's count is obtained (pg_filter_stats.h)
  fstats::Plan stats_plan = fstats::Plan::kZero;
  int stats_scan_leaves = 0;
  bool stats_chain_flagged = false;            // the chain's scan leaves carry kNodeCountEntries
  bool stats_leap2_flagged = false;            // the root AND of two scan leaves carries kNodeLeapfrog2
  bool plane_pending = false;                  // a value plane this query wanted is still being built (or had no room): the lowering is not the one to keep
  bool cardinality_only_hint = false;          // in: the query is COUNT(*) only, so an index-only filter needs neither bitmap nor tile list
  // index_and_finalize_kernel (window masks -> the ascending tile list, its length, the cardinality) is launched only when somebody reads its
  // output: scan_sparse_kernel walks the window masks themselves and COUNT(*) takes the cardinality from index_and_kernel's own counter
  bool finalize_pending = false;
  unsigned finalize_windows = 0;
  // index_and_kernel itself is launched when the planner knows what follows it (launch_index_and): a COUNT(*) wants its cardinality counters,
  // an aggregation over a handful of survivors per window is done INSIDE it (gathered: no bitmap, no second kernel), everything else its
  // bitmap and window masks.  Lowering only prepares the kernel's arguments.
  bool and_pending = false, and_cardinality_only = false, gathered = false;
  // dictId-set leaves (IN lists): where the words were uploaded for THIS context, and the host's copy -- a batch's shared launch reads them
  // from the batch's own blob instead (enqueue_deferred), so such an item is not tied to a context
  struct SetLeaf { const uint32_t* ctx_words; const uint32_t* host_words; uint32_t bytes; };
  std::vector<SetLeaf> set_leaves;
  bool cardinality_atomic = false;             // index_and_kernel added its figures to the context's counter lines (launch_index_and; read_index_and_shards)
  int and_num_cus = 256;                       // the segment's CUs (pg_segment.num_cus): index_and_kernel's persistent grid is sized by them
  IndexAndParams and_params;
  double and_expected_docs = 0;                // the planner's estimate of the AND's cardinality (independent postings)
  FsmSide* side = nullptr;                     // in: the transducer pass wants the leaves' bitmaps (ScanParams.leaf_out)
  // PG_PRED_RAW_SET leaves.  in: the query has the shape of scan_raw_set_kernel (raw_set_lean_shape), so its one leaf stays a kLeafRawSet; every
  // other query gets the leaf's match bitmap from raw_set_bitmap_kernel ahead of its kernel.  The host tables live as long as the lowering.
  bool raw_set_lean_hint = false;
  std::vector<std::shared_ptr<RawSetTable>> raw_set_tables;
  // PG_PRED_DOC_SET leaves: the sets whose words the lowered filter reads, held for as long as the lowering lives.  valid_leaf: the index
  // (PlanParams.leaves) of a NON-exclusive doc-set leaf, the one scan_simple_valid_kernel may take; -1: none.
  std::vector<std::shared_ptr<DocSet>> doc_sets;
  int valid_leaf = -1;
  int64_t stats_closed_entries = -1;           // >= 0: numEntriesScannedInFilter as a closed form (scan_simple_valid_kernel: the doc set's cardinality)
  uint32_t* sp_leaf_out[kMaxLeaves] = {};      // out: ScanParams.leaf_out, by LEAF node ordinal
  // the bitset pass of a DISTINCTCOUNT query (kQueryDistinctPass): plan slots of its DISTINCTCOUNT columns and of group_distinct_kernel's keys
  std::vector<int> distinct_slots, distinct_key_slots;
  bool hll_pass = false;                       // kQueryHllPass: the slots are RAW columns with a log2m each (hll_slot_log2m), the kernels scan_hll_kernel / group_hll_kernel (pg_scan_hll.h)
  std::vector<int> hll_slot_log2m;
  bool moments_pass = false;                   // kQueryMomentsPass: the slots are VARIANCE columns, raw or dictionary-encoded, the kernels scan_moments_kernel / group_moments_kernel (pg_scan_moments.h)
  bool counts_pass = false;                    // kQueryCountsPass: the slots are PERCENTILE columns, the kernels scan_counts_kernel / group_counts_kernel (32-bit counters per dictId)
  bool collect_pass = false;                   // kQueryCollectPass: the slots are RAW columns, the kernels scan_collect_kernel / group_collect_kernel (pg_scan_collect.h)
};

int slot_for(Lowered* lw, const pg_segment* seg, int column, bool plane = false) {
  const int id = column * 2 + (plane ? 1 : 0);
  for (size_t i = 0; i < lw->col_of_slot.size(); ++i) if (lw->col_of_slot[i] == id) return (int)i;
  if ((int)lw->col_of_slot.size() >= kMaxCols) return -1;
  const ColumnDev& c = seg->cols[column];
  DevColumn& d = lw->plan.cols[lw->col_of_slot.size()];
  memset(&d, 0, sizeof(d));
  if (plane && c.vkind != kValI32) {
    // wide plane of a LONG / DOUBLE dictionary column: the values themselves, big-endian 8 bytes per doc -- the image of a raw column
    d.fwd = c.d_plane;
    d.dict = nullptr;
    d.bits = 32;
    d.is_raw = 1;
    d.is_plane = 0;
    d.vkind = c.vkind;
  } else if (plane) {
    d.fwd = c.d_plane;
    d.dict = nullptr;
    d.bits = c.plane_bits;
    d.is_raw = c.plane_bits == 32;     // 32-bit planes are big-endian int32 values: the raw-column path
    d.is_plane = c.plane_bits == 32 ? 0 : 1;
    d.cardinality = 0;
    d.dict_bytes = 0;
  } else {
    d.fwd = c.d_fwd;
    d.dict = c.vkind == kValI32 ? c.d_dict : reinterpret_cast<const int32_t*>(c.d_dict64);
    d.bits = c.encoding == PG_FWD_RAW_FIXED_BYTE ? 32 : c.bits;
    d.is_raw = c.encoding == PG_FWD_RAW_FIXED_BYTE;
    d.cardinality = c.cardinality;
    d.dict_bytes = c.cardinality * (c.vkind == kValI32 ? 4 : 8);
    d.vkind = c.vkind;
  }
  if (!d.is_raw) lw->max_bits = std::max(lw->max_bits, d.bits);
  lw->col_of_slot.push_back(id);
  lw->plan.num_cols = (int)lw->col_of_slot.size();
  return lw->plan.num_cols - 1;
}

struct SeqNode { int src; int op; int num_children; int flags; };

// Re-orders the children of a root AND so that inverted-index (bitmap) leaves come first, rewrites that AND as a chain
// of binary ANDs flagged kNodeExitIfZero (AND is commutative and associative: same docId set), and reports where the
// bitmap prefix ends.  Everything else keeps its postfix order.
constexpr int kSeqIndexAnd = -2;       // SeqNode.src of the leaf that stands for all inverted-index children of the root AND

bool is_inverted_leaf(const pg_query* q, int node) {
  if (q->filter[node].op != PG_FILTER_LEAF) return false;
  const int pi = q->filter[node].predicate;
  if (pi < 0 || pi >= q->num_predicates) return false;
  const pg_predicate& pr = q->predicates[pi];
  return pr.eval == PG_EVAL_INVERTED && (pr.kind == PG_PRED_DICT_RANGE || pr.kind == PG_PRED_DICT_SET);
}

void build_sequence(const pg_query* q, std::vector<SeqNode>* seq, int* lazy_node, int* num_bitmap_prefix, std::vector<int>* and_members) {
  const int n = q->num_filter_nodes;
  *lazy_node = -1;
  *num_bitmap_prefix = 0;
  seq->clear();
  and_members->clear();
  if (n == 0) return;
  std::vector<int> start((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    const pg_filter_node& fn = q->filter[i];
    if (fn.op == PG_FILTER_LEAF) start[(size_t)i] = i;
    else {
      int k = fn.op == PG_FILTER_NOT ? 1 : fn.num_children;
      int idx = i - 1;
      for (int c = 0; c < k && idx >= 0; ++c) idx = start[(size_t)idx] - 1;
      start[(size_t)i] = idx + 1;
    }
  }
  const pg_filter_node& root = q->filter[n - 1];
  auto identity = [&](int from, int to) { for (int i = from; i <= to; ++i) seq->push_back(SeqNode{i, q->filter[i].op, q->filter[i].num_children, 0}); };
  if (root.op != PG_FILTER_AND || root.num_children < 2 || start[(size_t)n - 1] != 0) {
    if (n == 1 && is_inverted_leaf(q, 0)) {
      // a single inverted-index leaf: the same window-by-window kernel expands it and lists the tiles that hold a match
      and_members->push_back(q->filter[0].predicate);
      seq->push_back(SeqNode{kSeqIndexAnd, PG_FILTER_LEAF, 0, kNodeExitIfZero});
      return;
    }
    identity(0, n - 1);
    if (root.op == PG_FILTER_LEAF) seq->back().flags |= kNodeExitIfZero;
    return;
  }
  // children of the root, in query order
  std::vector<std::pair<int, int>> children;   // [first, last] node index of each child subtree
  int idx = n - 2;
  for (int c = 0; c < root.num_children; ++c) { children.push_back({start[(size_t)idx], idx}); idx = start[(size_t)idx] - 1; }
  std::reverse(children.begin(), children.end());
  auto is_bitmap_leaf = [&](const std::pair<int, int>& ch) {
    if (ch.first != ch.second || q->filter[ch.first].op != PG_FILTER_LEAF) return false;
    const int pi = q->filter[ch.first].predicate;
    if (pi < 0 || pi >= q->num_predicates) return false;
    const pg_predicate& pr = q->predicates[pi];
    // index-driven leaves go first, like the reference's priorities (sorted 0 < bitmap 100 < scan 500, FilterOperatorUtils.java:205-251)
    return pr.kind == PG_PRED_DOC_RANGE || pr.kind == PG_PRED_IS_NULL || pr.kind == PG_PRED_DOC_SET ||
           (pr.eval == PG_EVAL_INVERTED && (pr.kind == PG_PRED_DICT_RANGE || pr.kind == PG_PRED_DICT_SET));
  };
  std::stable_partition(children.begin(), children.end(), is_bitmap_leaf);
  // The inverted-index children are and-ed by ONE kernel, container by container (AndDocIdSet.java:127-165 and-s the index-based
  // children first): they become a single leaf at the head of the chain.
  std::vector<std::pair<int, int>> rest;
  for (const auto& ch : children) {
    if (ch.first == ch.second && is_inverted_leaf(q, ch.first) && (int)and_members->size() < kMaxAndChildren) and_members->push_back(q->filter[ch.first].predicate);
    else rest.push_back(ch);
  }
  const int head = and_members->empty() ? 0 : 1;
  for (const auto& ch : rest) *num_bitmap_prefix += is_bitmap_leaf(ch) ? 1 : 0;
  *num_bitmap_prefix += head;
  for (size_t c = 0; c < rest.size() + (size_t)head; ++c) {
    if (head && c == 0) seq->push_back(SeqNode{kSeqIndexAnd, PG_FILTER_LEAF, 0, 0});
    else identity(rest[c - (size_t)head].first, rest[c - (size_t)head].second);
    if (c == 0) seq->back().flags |= kNodeExitIfZero;
    else seq->push_back(SeqNode{-1, PG_FILTER_AND, 2, kNodeExitIfZero});
    if ((int)c + 1 == *num_bitmap_prefix) *lazy_node = (int)seq->size() - 1;
  }
}

// kNodeCountEntries leaves: the device counter the lane-private kernels add their entries to, zeroed in stream order.
// Timed runs (PG_CFG_TIME_KERNELS): ev[0] opens the query's device work.  It is recorded by the first thing that enqueues work BEFORE
// the scan kernel (index AND, posting expansion, set uploads, table initialisation); a query that runs only its scan kernel opens with ev[1].
hipError_t mark_pre_work(ExecCtx* ctx) {
  ctx->pre_enqueued = true;          // (pg_execute_batch: such a query runs on its own context, not in the shared launch)
  if (!(g_engine.flags & PG_CFG_TIME_KERNELS) || ctx->pre_started) return hipSuccess;
  ctx->pre_started = true;
  return hipEventRecord(ctx->ev[0], ctx->stream);
}

pg_status arm_filter_entries(ExecCtx* ctx, unsigned long long** out_counter) {
  if (!ctx->d_filter_entries) HIP_TRY(hipMalloc((void**)&ctx->d_filter_entries, 8));
  if (!ctx->h_filter_entries) HIP_TRY(hipHostMalloc((void**)&ctx->h_filter_entries, 8, hipHostMallocDefault));
  HIP_TRY(mark_pre_work(ctx));
  HIP_TRY(hipMemsetAsync(ctx->d_filter_entries, 0, 8, ctx->stream));
  *out_counter = ctx->d_filter_entries;
  return PG_OK;
}

// Zeros in every tile index_and_kernel did not store: for the kernels that read the whole bitmap instead of the tile list.
// kNodeLeapfrog2: the per-tile bytes, the per-1024-tile summaries, and the (zeroed) entries counter the kernels and the chain add to
pg_status arm_leap_tables(const pg_segment* seg, ExecCtx* ctx, uint8_t** out_tables, unsigned long long** out_counter /* nullptr: the scan kernel's record carries the count */) {
  const size_t tiles = (size_t)std::max(seg->num_tiles, 1);
  if (ctx->leap_capacity < tiles) {
    if (ctx->d_leap_tables) (void)hipFree(ctx->d_leap_tables);
    ctx->d_leap_tables = nullptr; ctx->d_leap_blocks = nullptr; ctx->leap_capacity = 0;
    const size_t table_bytes = (tiles + 255) & ~(size_t)255;
    HIP_TRY(hipMalloc((void**)&ctx->d_leap_tables, table_bytes + ((tiles + 1023) / 1024) * sizeof(Leap2Summary)));
    ctx->d_leap_blocks = reinterpret_cast<Leap2Summary*>(ctx->d_leap_tables + table_bytes);
    ctx->leap_capacity = tiles;
  }
  *out_tables = ctx->d_leap_tables;
  return out_counter ? arm_filter_entries(ctx, out_counter) : PG_OK;
}

// behind the scan kernel: the entry states of the tiles, chained in tile order, decide which tiles' corrections count.  The result goes
// into the context's pinned record (host_seq != 0: aggregation queries) or onto the device counter (group-by queries).
pg_status launch_leap_chain(const pg_segment* seg, ExecCtx* ctx, unsigned long long host_seq) {
  const long long tiles = ((long long)seg->num_docs + 2047) / 2048;
  const int blocks = (int)std::max<long long>(1, (tiles + 1023) / 1024);
  leapfrog2_chain_kernel<<<dim3((unsigned)blocks), dim3(1024), 0, ctx->stream>>>(ctx->d_leap_tables, tiles, ctx->d_leap_blocks, ctx->d_done + (kFoldShards + 1) * kFoldStride,
                                                                                  host_seq ? ctx->h_record_dev : nullptr, host_seq, host_seq ? nullptr : ctx->d_filter_entries);
  HIP_TRY(hipGetLastError());
  return PG_OK;
}

// The aggregation INSIDE index_and_kernel: ScanParams.agg_cols are the columns it reads; no bitmap is stored.
static void arm_index_gather(Lowered* lw, const ScanParams* gather_from) {
  IndexAndParams& ap = lw->and_params;
  ap.gather_cols = gather_from->num_agg_cols;
  for (int a = 0; a < gather_from->num_agg_cols && a < kMaxAndGather; ++a) ap.gather_col[a] = gather_from->agg_cols[a];
  ap.out = nullptr;                              // nobody reads a bitmap
  lw->gathered = true;
}
// pg_execute_batch: an index-led item whose whole device work is index_and_kernel publishing the query's record -- COUNT(*) over the whole
// filter, or the gathered aggregation -- can share index_and_batch_kernel's launch when nothing of it lives in the lowering context:
// no child expanded densely ahead of the kernel (such a child is a bitmap of the context, and a launch of its own before this one).
static bool index_and_shares_a_launch(const Lowered& lw) {
  if (!lw.and_pending || lw.finalize_windows == 0) return false;
  for (int c = 0; c < lw.and_params.num_children; ++c) if (lw.and_params.child[c].dense != nullptr) return false;
  return true;
}

// index_and_kernel, launched when its consumer is known.  `gather_from`: the aggregation runs inside the kernel (ScanParams.agg_cols are the
// columns it reads; no bitmap is stored); else the kernel leaves its bitmap / window masks.  COUNT(*) over the whole filter and the gathered
// aggregation come back on the context's counter lines (IndexAndParams.shards): the caller copies them to ctx->h_and_shards, reads them
// with read_index_and_shards and zeroes them again behind the answer.
pg_status launch_index_and(Lowered* lw, ExecCtx* ctx, const ScanParams* gather_from) {
  if (!lw->and_pending) return PG_OK;
  lw->and_pending = false;
  IndexAndParams& ap = lw->and_params;
  const unsigned num_windows = lw->finalize_windows;
  // One wavefront per workgroup; a wave takes windows key, key + grid, ... with the next window's directory lookups in flight
  // (pg_index_and.h).  PINOT_GPU_INDEX_AND_WAVES: 0 (default) = a persistent grid of as many waves as are resident; n > 0 = of n waves per
  // CU; -k = k windows per wave (grid = windows / k workgroups handed out by the dispatcher as slots free up; -1: a wave per window, rounds
  // 2-5).  Measured on C5 at 1 B rows (profiles/r6/c5_index_and_*.jsonl): the kernel is bound by instruction issue, not by waiting (SQ
  // counters: the waves' active-instruction cycles per SIMD add up to the kernel's duration), so the grid's shape moves it by a few
  // percent only -- after the scalar-instruction diet the resident grid is ahead (COUNT 39.5 vs 43.3 us, gathered SUM 58.1 vs 58.5-59.6);
  // 8 or 12 waves per CU lose 20 - 40 %.
  const int per_cu = g_engine.index_and_waves > 0 ? g_engine.index_and_waves : waves_index_and();
  const unsigned grid = g_engine.index_and_waves < 0 ? (num_windows + (unsigned)(-g_engine.index_and_waves) - 1) / (unsigned)(-g_engine.index_and_waves)
                                                      : (unsigned)std::min<long long>(num_windows, (long long)lw->and_num_cus * per_cu);
  memset(&ap.pub, 0, sizeof(ap.pub));
  ap.shards = nullptr;
  ap.num_windows = (int32_t)num_windows;
  if (gather_from != nullptr) arm_index_gather(lw, gather_from);
  if (lw->and_cardinality_only || gather_from != nullptr) {
    // the wavefronts add what they found to counter lines the host keeps at zero between queries
    if (ctx->and_counter_dirty) HIP_TRY(hipMemsetAsync(ctx->d_and_counters + 2, 0, kAndShardBytes, ctx->stream));      // (a query that failed before it read them)
    ap.shards = ctx->d_and_counters + 2;
    ctx->and_counter_dirty = true;
    lw->cardinality_atomic = true;
  }
  if (num_windows) {
    launch_index_and_kernel((int)grid, ctx->stream, ap, num_windows);
    HIP_TRY(hipGetLastError());
    // (index_and_finalize_kernel: only when the tile list is read -- complete_index_list)
    lw->finalize_pending = !lw->and_cardinality_only && gather_from == nullptr;
  } else if (!lw->and_cardinality_only && gather_from == nullptr) {
    HIP_TRY(hipMemsetAsync(ctx->d_and_counters, 0, 16, ctx->stream));
  }
  return PG_OK;
}
// The counter lines of a COUNT(*) / gathering index_and_kernel, copied to ctx->h_and_shards and complete (the stream was waited for): zeroes
// the device's lines again behind the answer (nobody waits for that) and folds the 64 lines into one record.
pg_status read_index_and_shards(ExecCtx* ctx, int gather_cols, BlockPartial* g) {
  HIP_TRY(hipMemsetAsync(ctx->d_and_counters + 2, 0, kAndShardBytes, ctx->stream));
  ctx->and_counter_dirty = false;
  memset(g, 0, sizeof(*g));
  for (int a = 0; a < kMaxAggCols; ++a) { g->kmin[a] = 0x7FFFFFFF; g->kmax[a] = (int32_t)0x80000000; }
  const unsigned long long* lines = ctx->h_and_shards;
  unsigned long long kmin_inv[kMaxAndGather] = {0ull, 0ull}, kmax[kMaxAndGather] = {0ull, 0ull};
  for (int sh = 0; sh < kAndCardinalityShards; ++sh) {
    const unsigned long long* line = lines + (size_t)sh * 16;
    g->count += line[0];
    for (int a = 0; a < gather_cols && a < kMaxAndGather; ++a) {
      g->sum[a] += (long long)line[1 + 3 * a];
      kmin_inv[a] = std::max(kmin_inv[a], line[2 + 3 * a]);
      kmax[a] = std::max(kmax[a], line[3 + 3 * a]);
    }
  }
  for (int a = 0; a < gather_cols && a < kMaxAndGather; ++a) {
    if (g->count == 0ull) continue;                 // (identities stay)
    g->kmin[a] = (int32_t)(0xFFFFFFFFull - kmin_inv[a]);
    g->kmax[a] = (int32_t)kmax[a];
  }
  return PG_OK;
}

// The tile list of an index-led filter, for the kernels that read one (everything but scan_sparse_kernel): index_and_finalize_kernel behind
// index_and_kernel, on the query's stream, the first time the list is asked for.
pg_status complete_index_list(Lowered* lw, ExecCtx* ctx) {
  { const pg_status ls = launch_index_and(lw, ctx, nullptr); if (ls != PG_OK) return ls; }
  if (!lw->finalize_pending) return PG_OK;
  lw->finalize_pending = false;
  index_and_finalize_kernel<<<dim3((lw->finalize_windows + 255) / 256), dim3(256), 0, ctx->stream>>>(ctx->d_window_info, (int)lw->finalize_windows, ctx->d_tile_list,
                                                                                                    reinterpret_cast<uint32_t*>(ctx->d_and_counters + 1), ctx->d_and_counters);
  HIP_TRY(hipGetLastError());
  return PG_OK;
}

pg_status complete_index_and_bitmap(Lowered* lw, ExecCtx* ctx) {
  { const pg_status ls = launch_index_and(lw, ctx, nullptr); if (ls != PG_OK) return ls; }
  if (!lw->and_bitmap) return PG_OK;
  HIP_TRY(mark_pre_work(ctx));
  index_and_zero_unlisted_kernel<<<dim3(2048), dim3(256), 0, ctx->stream>>>(lw->and_info, lw->and_bitmap, lw->and_words);
  HIP_TRY(hipGetLastError());
  lw->and_bitmap = nullptr;
  return PG_OK;
}

static std::shared_ptr<DocSet> find_doc_set(const pg_segment* seg, int64_t id) {
  std::lock_guard<std::mutex> lk(seg->doc_sets_mu);
  for (const auto& ds : seg->doc_sets) if (ds->id == id) return ds;
  return nullptr;
}

// PG_PRED_RAW_SET (include/pinot_gpu.h): the argument checks and the declines, the same for pg_query_check and pg_execute.  *keys: the
// distinct members as bit patterns of the column's own type (empty: the leaf matches nothing).
static pg_status check_raw_set(const pg_segment* seg, const pg_predicate& pr, std::vector<uint64_t>* keys) {
  if (pr.column < 0 || pr.column >= (int)seg->cols.size()) return fail(PG_ERR_INVALID_ARGUMENT, "predicate column %d out of range", pr.column);
  const ColumnDev& col = seg->cols[(size_t)pr.column];
  if (col.encoding == PG_FWD_FIXED_BIT_DICT) return fail(PG_ERR_INVALID_ARGUMENT, "raw predicate on dictionary column %s", col.name.c_str());
  if (pr.eval != PG_EVAL_SCAN) return fail(PG_ERR_INVALID_ARGUMENT, "a raw value set on column %s is a scan leaf (eval %d)", col.name.c_str(), pr.eval);
  if (pr.num_set_words < 0 || (pr.num_set_words & 1) || (pr.num_set_words > 0 && !pr.set_words))
    return fail(PG_ERR_INVALID_ARGUMENT, "bad raw value set on column %s: %d words (two per value)", col.name.c_str(), pr.num_set_words);
  const int rc = decode_raw_set_words(col.stored_type, pr.set_words, pr.num_set_words, keys);
  if (rc == 1) return fail(PG_ERR_UNSUPPORTED, "IN list on raw column %s holds a zero or a NaN: how the reference's hash set treats them is not settled -- CPU plan", col.name.c_str());
  if (rc == 2) return fail(PG_ERR_UNSUPPORTED, "IN list on raw column %s has %zu distinct values (max %d)", col.name.c_str(), keys->size(), kRawSetMaxValues);
  return PG_OK;
}
static int raw_set_key_bytes(const ColumnDev& col) { return (col.stored_type == PG_TYPE_INT || col.stored_type == PG_TYPE_FLOAT) ? 4 : 8; }

// The shape scan_raw_set_kernel takes (the test choose_scan_kernel applies for scan_raw_kernel, on the query itself: the leaf's device form
// is decided while the filter is lowered): the whole filter is ONE raw-set leaf, no group-by, no bitmap wanted, and at most one aggregated
// column, a raw INT one.
static bool raw_set_lean_shape(const pg_segment* seg, const pg_query* q, int na, int ng, bool want_bitmap, bool want_result) {
  if (!g_engine.scan_raw_set || ng != 0 || want_bitmap || !want_result || (g_engine.flags & PG_CFG_PROFILE_WAVES)) return false;
  if (q->num_filter_nodes != 1 || q->filter[0].op != PG_FILTER_LEAF || q->filter[0].predicate < 0 || q->filter[0].predicate >= q->num_predicates) return false;
  if (q->predicates[q->filter[0].predicate].kind != PG_PRED_RAW_SET) return false;
  int only = -1;
  for (int a = 0; a < na; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    if (ag.function == PG_AGG_COUNT) continue;
    if (ag.column < 0 || ag.column >= (int)seg->cols.size() || (only >= 0 && only != ag.column)) return false;
    const ColumnDev& c = seg->cols[(size_t)ag.column];
    if (c.encoding != PG_FWD_RAW_FIXED_BYTE || c.stored_type != PG_TYPE_INT || c.vkind != kValI32) return false;
    only = ag.column;
  }
  return true;
}

pg_status lower_filter(pg_segment* seg, ExecCtx* ctx, const pg_query* q, Lowered* lw) {
  PlanParams& sp = lw->plan;
  if (q->num_filter_nodes < 0 || q->num_filter_nodes > kMaxNodes) return fail(PG_ERR_UNSUPPORTED, "filter tree has %d nodes (max %d)", q->num_filter_nodes, kMaxNodes);
  if (q->num_filter_nodes > 0 && (!q->filter || !q->predicates)) return fail(PG_ERR_INVALID_ARGUMENT, "filter nodes without predicates");
  for (int n = 0; n < q->num_filter_nodes; ++n) {
    const int op = q->filter[n].op;
    if (op < PG_FILTER_LEAF || op > PG_FILTER_NOT) return fail(PG_ERR_INVALID_ARGUMENT, "unknown filter op %d", op);
    if ((op == PG_FILTER_AND || op == PG_FILTER_OR) && q->filter[n].num_children < 1) return fail(PG_ERR_INVALID_ARGUMENT, "malformed filter tree (node %d)", n);
  }
  std::vector<SeqNode> seq;
  std::vector<int> and_members;
  int lazy_node = -1, num_bitmap_prefix = 0;
  build_sequence(q, &seq, &lazy_node, &num_bitmap_prefix, &and_members);
  for (int pi : and_members) if (pi < 0 || pi >= q->num_predicates) return fail(PG_ERR_INVALID_ARGUMENT, "bad predicate index");
  // InvertedIndexFilterOperator.getTrues as a dense doc-order bitmap: OR of the postings of every matching dictId (the general path:
  // leaves under OR / NOT, and members of the index AND with more than kMaxAndPostings postings)
  auto expand_dense = [&](const ColumnDev& col, const pg_predicate& pr, unsigned long long* bm) -> pg_status {
    const long long words = (long long)seg->num_tiles * kMaxTileSteps;
    const unsigned num_windows = (unsigned)((words + 1023) / 1024);
    bool first_posting = true;
    HIP_TRY(mark_pre_work(ctx));
    for (int d = 0; d < col.cardinality; ++d) {
      bool in;
      if (pr.kind == PG_PRED_DICT_RANGE) in = d >= pr.lo && d < pr.hi;
      else in = (d >> 5) < pr.num_set_words && ((pr.set_words[d >> 5] >> (d & 31)) & 1u);
      if (!in) continue;
      const int64_t first = col.posting_first[d], cnt = col.posting_first[d + 1] - first;
      if (cnt <= 0 && !first_posting) continue;
      // the first posting stores every window (zeros where it has no container); later ones OR
      roaring_expand_kernel<<<dim3(num_windows), dim3(kBlockThreads), 0, ctx->stream>>>(col.d_inv, col.d_dir, (int)first, (int)cnt, bm, words, first_posting ? 0 : 1);
      first_posting = false;
    }
    if (first_posting) fill_words_kernel<<<dim3(256), dim3(256), 0, ctx->stream>>>(bm, words, 0ull);   // no dictId matched
    HIP_TRY(hipGetLastError());
    return PG_OK;
  };
  if ((int)seq.size() > kMaxNodes) return fail(PG_ERR_UNSUPPORTED, "filter tree has %d nodes (max %d)", (int)seq.size(), kMaxNodes);
  int depth = 0, max_depth = 0;
  size_t bitmap_idx = 1;   // bitmap 0 is reserved for pg_filter_bitmap output
  size_t set_idx = 0;
  for (int n = 0; n < (int)seq.size(); ++n) {
    pg_filter_node fn;
    memset(&fn, 0, sizeof(fn));
    if (seq[(size_t)n].src >= 0) fn = q->filter[seq[(size_t)n].src];
    fn.op = seq[(size_t)n].op;
    fn.num_children = seq[(size_t)n].num_children;
    PlanNode& dn = sp.nodes[n];
    dn.op = fn.op;
    dn.leaf = -1;
    dn.num_children = fn.num_children;
    dn.flags = seq[(size_t)n].flags;
    if (lw->side != nullptr) {
      // every leaf's mask of every tile feeds the walk: no leaf may end a tile early; a leaf that is one of the walk's inputs stores its mask
      dn.flags &= ~kNodeExitIfZero;
      if (fn.op == PG_FILTER_LEAF) {
        int ordinal = 0;
        for (int m = 0; m < n; ++m) ordinal += seq[(size_t)m].op == PG_FILTER_LEAF ? 1 : 0;
        if (seq[(size_t)n].src >= 0 && ordinal < kMaxLeaves) {
          const std::vector<int>& inputs = lw->side->fsm->input_predicate;
          for (size_t i = 0; i < inputs.size(); ++i) {
            if (inputs[i] != fn.predicate || lw->side->mapped[i]) continue;
            lw->sp_leaf_out[ordinal] = lw->side->bitmap[i];
            lw->side->mapped[i] = true;
          }
        }
      }
    }
    if (lw->stats_plan == fstats::Plan::kLeap2) {
      // `a AND b`, two scan leaves: both masks of EVERY tile feed the leap-frog entry count, so no leaf may end a tile early
      // (whichever leaf is scanning when a tile is entered keeps looking at its docs even where the other one matches nothing)
      if (fn.op == PG_FILTER_LEAF) dn.flags &= ~kNodeExitIfZero;
      else if (fn.op == PG_FILTER_AND && n == (int)seq.size() - 1 && seq.size() == 3) { dn.flags |= kNodeLeapfrog2; lw->stats_leap2_flagged = true; }
    }
    if (lw->stats_plan == fstats::Plan::kChain && fn.op == PG_FILTER_LEAF && seq[(size_t)n].src >= 0 && fn.predicate >= 0 && fn.predicate < q->num_predicates &&
        fstats::classify(q->predicates[fn.predicate]) == fstats::LeafClass::kScan && n > 0) {
      // a scan-based child of the root AND, behind the index-based ones: ScanBasedDocIdIterator.applyAnd looks at every doc still standing
      dn.flags |= kNodeCountEntries;
      lw->stats_chain_flagged = true;
    }
    if (fn.op == PG_FILTER_LEAF && seq[(size_t)n].src == kSeqIndexAnd) {
      // ---- the inverted-index children of the root AND, intersected container by container (index_and_kernel) ----
      if (sp.num_leaves >= kMaxLeaves) return fail(PG_ERR_UNSUPPORTED, "more than %d filter leaves", kMaxLeaves);
      DevLeaf& L = sp.leaves[sp.num_leaves];
      memset(&L, 0, sizeof(L));
      dn.leaf = sp.num_leaves++;
      struct Member { AndChild child; double estimate; std::vector<std::pair<int32_t, int32_t>> postings; };
      std::vector<Member> members;
      bool empty = false;
      for (int pi : and_members) {
        const pg_predicate& pr = q->predicates[pi];
        if (pr.column < 0 || pr.column >= (int)seg->cols.size()) return fail(PG_ERR_INVALID_ARGUMENT, "predicate column %d out of range", pr.column);
        const ColumnDev& col = seg->cols[pr.column];
        if (col.encoding != PG_FWD_FIXED_BIT_DICT) return fail(PG_ERR_INVALID_ARGUMENT, "dictionary predicate on raw column %s", col.name.c_str());
        if (!col.d_inv) return fail(PG_ERR_INVALID_ARGUMENT, "column %s has no inverted index", col.name.c_str());
        if (pr.kind == PG_PRED_DICT_SET && (pr.num_set_words < 0 || (pr.num_set_words > 0 && !pr.set_words))) return fail(PG_ERR_INVALID_ARGUMENT, "bad dictId set");
        Member mb;
        memset(&mb.child, 0, sizeof(mb.child));
        mb.child.inv = col.d_inv; mb.child.dir = col.d_dir; mb.child.exclusive = pr.exclusive ? 1 : 0;
        double docs = 0;
        int postings = 0;
        // (a range walks its own dictIds only, a set the dictIds its words can name)
        const bool is_range = pr.kind == PG_PRED_DICT_RANGE;
        const int d_begin = is_range ? (int)std::max<int64_t>(pr.lo, 0) : 0;
        const int d_end = is_range ? (int)std::min<int64_t>(pr.hi, col.cardinality) : (int)std::min<int64_t>((int64_t)pr.num_set_words * 32, col.cardinality);
        for (int d = d_begin; d < d_end; ++d) {
          if (!is_range && !((pr.set_words[d >> 5] >> (d & 31)) & 1u)) continue;
          const int64_t first = col.posting_first[d], cnt = col.posting_first[d + 1] - first;
          if (cnt <= 0) continue;
          docs += (double)col.posting_docs[(size_t)d];
          if (postings < kMaxChildPostings) mb.postings.emplace_back((int32_t)first, (int32_t)cnt);
          postings++;
        }
        if (postings == 0 && !pr.exclusive) { empty = true; break; }          // nothing matches this child: the AND is empty
        if (postings == 0 && pr.exclusive) continue;                          // NOT (nothing) = everything: the child drops out
        mb.estimate = pr.exclusive ? (double)seg->num_docs - docs : docs;
        size_t inline_so_far = 0;
        for (const Member& m : members) inline_so_far += m.postings.size();
        if (postings > kMaxChildPostings || inline_so_far + (size_t)postings > (size_t)kMaxAndPostings) {
          // too many postings for one lookup per lane: this child is expanded densely first
          pg_status st = ensure_bitmap(seg, ctx, bitmap_idx);
          if (st != PG_OK) return st;
          unsigned long long* bm = ctx->d_bitmaps[bitmap_idx++];
          st = expand_dense(col, pr, bm);
          if (st != PG_OK) return st;
          mb.child.inv = nullptr; mb.child.dir = nullptr; mb.child.dense = bm;
          mb.postings.clear();
        }
        members.push_back(std::move(mb));
      }
      if (empty) { L.kind = kLeafMatchNone; depth++; max_depth = std::max(max_depth, depth); continue; }
      if (members.empty()) { L.kind = kLeafMatchAll; depth++; max_depth = std::max(max_depth, depth); continue; }
      // smallest first, like AndDocIdSet sorts its bitmaps: an empty window ends the work for the later children
      std::stable_sort(members.begin(), members.end(), [](const Member& a, const Member& b) { return a.estimate < b.estimate; });
      const bool cardinality_only = lw->cardinality_only_hint && seq.size() == 1;     // FastFilteredCount: neither the bitmap nor the tile list is read
      unsigned long long* bm = nullptr;
      if (!cardinality_only) {
        pg_status st = ensure_bitmap(seg, ctx, bitmap_idx);
        if (st != PG_OK) return st;
        bm = ctx->d_bitmaps[bitmap_idx++];
      }
      const long long num_words = (long long)seg->num_tiles * kMaxTileSteps;
      const unsigned num_windows = (unsigned)((num_words + 1023) / 1024);
      if (ctx->tile_list_capacity < (size_t)seg->num_tiles + 64 || ctx->window_info_capacity < (size_t)num_windows + 1) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->d_tile_list) (void)hipFree(ctx->d_tile_list);
        if (ctx->d_window_info) (void)hipFree(ctx->d_window_info);
        ctx->d_tile_list = nullptr; ctx->d_window_info = nullptr;
        ctx->tile_list_capacity = (size_t)seg->num_tiles + 64;
        ctx->window_info_capacity = (size_t)num_windows + 1;
        HIP_TRY(hipMalloc((void**)&ctx->d_tile_list, ctx->tile_list_capacity * 4));
        HIP_TRY(hipMalloc((void**)&ctx->d_window_info, ctx->window_info_capacity * sizeof(WindowInfo)));
      }
      if (!ctx->d_and_counters) {
        // [0] cardinality and [1] tile count: index_and_finalize_kernel's outputs; behind them index_and_kernel's counter lines
        HIP_TRY(hipMalloc((void**)&ctx->d_and_counters, 16 + kAndShardBytes));
        HIP_TRY(hipMemsetAsync(ctx->d_and_counters, 0, 16 + kAndShardBytes, ctx->stream));
        HIP_TRY(hipHostMalloc((void**)&ctx->h_and_shards, kAndShardBytes, hipHostMallocDefault));
        ctx->and_counter_dirty = false;
      }
      IndexAndParams ap;
      memset(&ap, 0, sizeof(ap));
      ap.num_children = (int32_t)members.size();
      ap.num_docs = seg->num_docs;
      ap.num_words = num_words;
      ap.out = bm;
      ap.sparse_out = 1;
      ap.window_info = ctx->d_window_info;
      for (size_t c = 0; c < members.size(); ++c) {
        ap.child[c] = members[c].child;
        ap.child[c].posting_begin = ap.num_postings;
        for (const auto& ps : members[c].postings) {
          ap.first[ap.num_postings] = ps.first; ap.count[ap.num_postings] = ps.second; ap.posting_child[ap.num_postings] = (uint8_t)c;
          ap.num_postings++;
        }
        ap.child[c].posting_end = ap.num_postings;
      }
      unsigned long long* d_cardinality = ctx->d_and_counters;      // (index_and_finalize_kernel's; a cardinality-only or gathering launch publishes a record instead)
      uint32_t* d_tile_count = reinterpret_cast<uint32_t*>(ctx->d_and_counters + 1);
      HIP_TRY(mark_pre_work(ctx));
      // (the launch itself: launch_index_and, once the planner knows what reads the kernel's output)
      lw->and_params = ap;
      lw->and_num_cus = seg->num_cus;
      lw->and_pending = true;
      lw->and_cardinality_only = cardinality_only;
      lw->finalize_windows = num_windows;
      {
        double expected = (double)seg->num_docs;
        for (const Member& mb : members) expected *= std::min(1.0, std::max(0.0, (double)mb.estimate) / std::max(1.0, (double)seg->num_docs));
        lw->and_expected_docs = expected;
      }
      lw->d_cardinality = d_cardinality;
      lw->index_and_is_whole_filter = seq.size() == 1;
      if (cardinality_only) { L.kind = kLeafMatchAll; depth++; max_depth = std::max(max_depth, depth); continue; }   // never evaluated: execute_impl answers from the cardinality
      L.kind = kLeafBitmap;
      L.bitmap = bm;
      sp.num_bitmap_leaves++;
      lw->tile_list = ctx->d_tile_list;
      lw->tile_count = d_tile_count;
      lw->and_bitmap = bm;
      lw->and_info = ctx->d_window_info;
      lw->and_words = num_words;
      depth++;
      max_depth = std::max(max_depth, depth);
      continue;
    }
    if (fn.op == PG_FILTER_LEAF) {
      if (fn.predicate < 0 || fn.predicate >= q->num_predicates) return fail(PG_ERR_INVALID_ARGUMENT, "filter node %d: bad predicate index", n);
      if (sp.num_leaves >= kMaxLeaves) return fail(PG_ERR_UNSUPPORTED, "more than %d filter leaves", kMaxLeaves);
      const pg_predicate& pr = q->predicates[fn.predicate];
      DevLeaf& L = sp.leaves[sp.num_leaves];
      memset(&L, 0, sizeof(L));
      dn.leaf = sp.num_leaves++;
      L.exclusive = pr.exclusive ? 1 : 0;
      L.col = 0;
      if (pr.kind == PG_PRED_MATCH_ALL) { L.kind = kLeafMatchAll; }
      else if (pr.kind == PG_PRED_MATCH_NONE) { L.kind = kLeafMatchNone; }
      else if (pr.kind == PG_PRED_IS_NULL) {
        // FilterPlanNode.java:294-310: the null bitmap as a BitmapBasedFilterOperator; no null vector -> Empty (IS NULL) / MatchAll (IS NOT NULL)
        if (pr.column < 0 || pr.column >= (int)seg->cols.size()) return fail(PG_ERR_INVALID_ARGUMENT, "predicate column %d out of range", pr.column);
        const ColumnDev& col = seg->cols[pr.column];
        if (!col.d_null_bitmap) { L.kind = kLeafMatchNone; }
        else { L.kind = kLeafBitmap; L.bitmap = col.d_null_bitmap; sp.num_bitmap_leaves++; }
      }
      else if (pr.kind == PG_PRED_DOC_SET) {
        // FilterPlanNode.java:88-106: the queryable docIds as a BitmapBasedFilterOperator -- a kLeafBitmap over the doc set's words
        std::shared_ptr<DocSet> ds = find_doc_set(seg, pr.lo);
        if (!ds) return fail(PG_ERR_INVALID_ARGUMENT, "doc set %lld is unknown to segment %s (never created, or released)", (long long)pr.lo, seg->name.c_str());
        L.kind = kLeafBitmap; L.bitmap = ds->d_words; sp.num_bitmap_leaves++;
        if (!pr.exclusive && lw->valid_leaf < 0) lw->valid_leaf = dn.leaf;
        lw->doc_sets.push_back(std::move(ds));
      }
      else if (pr.kind == PG_PRED_DOC_RANGE) {
        // SortedIndexBasedFilterOperator: one inclusive docId range; nothing is scanned
        const int64_t lo = std::max<int64_t>(pr.lo, 0), hi = std::min<int64_t>(pr.hi, (int64_t)seg->num_docs - 1);
        if (lo > hi) L.kind = kLeafMatchNone;
        else { L.kind = kLeafDocRange; L.lo = (int32_t)lo; L.span = (uint32_t)(hi - lo); }
      }
      else {
        if (pr.column < 0 || pr.column >= (int)seg->cols.size()) return fail(PG_ERR_INVALID_ARGUMENT, "predicate column %d out of range", pr.column);
        const ColumnDev& col = seg->cols[pr.column];
        const bool is_dict = col.encoding == PG_FWD_FIXED_BIT_DICT;
        if ((pr.kind == PG_PRED_DICT_RANGE || pr.kind == PG_PRED_DICT_SET) && !is_dict)
          return fail(PG_ERR_INVALID_ARGUMENT, "dictionary predicate on raw column %s", col.name.c_str());
        if (pr.kind == PG_PRED_RAW_RANGE && is_dict) return fail(PG_ERR_INVALID_ARGUMENT, "raw predicate on dictionary column %s", col.name.c_str());
        if (pr.eval == PG_EVAL_INVERTED) {
          if (!col.d_inv) return fail(PG_ERR_INVALID_ARGUMENT, "column %s has no inverted index", col.name.c_str());
          if (pr.kind != PG_PRED_DICT_RANGE && pr.kind != PG_PRED_DICT_SET) return fail(PG_ERR_INVALID_ARGUMENT, "inverted-index leaf needs a dictionary predicate");
          // InvertedIndexFilterOperator.getTrues: OR of the postings of every matching dictId.
          if (pr.kind == PG_PRED_DICT_SET && (pr.num_set_words < 0 || (pr.num_set_words > 0 && !pr.set_words))) return fail(PG_ERR_INVALID_ARGUMENT, "bad dictId set");
          pg_status st = ensure_bitmap(seg, ctx, bitmap_idx);
          if (st != PG_OK) return st;
          unsigned long long* bm = ctx->d_bitmaps[bitmap_idx++];
          st = expand_dense(col, pr, bm);
          if (st != PG_OK) return st;
          L.kind = kLeafBitmap;
          L.bitmap = bm;
          sp.num_bitmap_leaves++;
        } else if (pr.kind == PG_PRED_DICT_RANGE) {
          int64_t lo = std::max<int64_t>(pr.lo, 0), hi = std::min<int64_t>(pr.hi, col.cardinality);
          if (lo >= hi) { L.kind = kLeafMatchNone; }
          else if (!lw->plane_cols.empty() && lw->plane_cols[(size_t)pr.column] && col.vkind == kValI32) {
            // The column is also summed through its value plane: evaluate the range on the plane so only one
            // stream is read.  The dictionary is sorted, so dictIds [lo, hi) <=> values [dict[lo], dict[hi-1]].
            int s = slot_for(lw, seg, pr.column, true);
            if (s < 0) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
            sp.cols[s].in_filter = 1;
            const int64_t vlo = col.h_dict[(size_t)lo], vhi = col.h_dict[(size_t)hi - 1];
            if (sp.cols[s].is_raw) { L.kind = kLeafRawRange; L.lo = (int32_t)vlo; L.span = (uint32_t)(vhi - vlo); }
            else { L.kind = kLeafDictRange; L.lo = (int32_t)((vlo - col.plane_base) / col.plane_scale); L.span = (uint32_t)((vhi - vlo) / col.plane_scale + 1); }
            L.col = s;
            lw->num_scan_leaves++;
          } else {
            int s = slot_for(lw, seg, pr.column);
            if (s < 0) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
            sp.cols[s].in_filter = 1;
            L.kind = kLeafDictRange; L.col = s; L.lo = (int32_t)lo; L.span = (uint32_t)(hi - lo);
            lw->num_scan_leaves++;
          }
        } else if (pr.kind == PG_PRED_DICT_SET) {
          if (pr.num_set_words < 0 || (pr.num_set_words > 0 && !pr.set_words)) return fail(PG_ERR_INVALID_ARGUMENT, "bad dictId set");
          int s = slot_for(lw, seg, pr.column);
          if (s < 0) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
          sp.cols[s].in_filter = 1;
          size_t bytes = (size_t)pr.num_set_words * 4;
          pg_status st = ensure_set(ctx, set_idx, bytes);
          if (st != PG_OK) return st;
          if (bytes) {
            // (the upload alone does not tie the query to this context: pg_execute_batch's shared launch carries the words itself)
            const bool tied = ctx->pre_enqueued;
            HIP_TRY(mark_pre_work(ctx));
            ctx->pre_enqueued = tied;
            HIP_TRY(hipMemcpyAsync(ctx->d_sets[set_idx], pr.set_words, bytes, hipMemcpyHostToDevice, ctx->stream));
            lw->set_leaves.push_back(Lowered::SetLeaf{ctx->d_sets[set_idx], pr.set_words, (uint32_t)bytes});
          }
          // the host words may go out of scope as soon as pg_execute returns; the copy is ordered before the kernel
          // on the same stream and the caller's buffer is read synchronously for pageable memory.
          L.kind = kLeafDictSet; L.col = s; L.set_words = ctx->d_sets[set_idx]; L.set_bytes = (int32_t)bytes;
          set_idx++;
          lw->num_scan_leaves++;
        } else if (pr.kind == PG_PRED_RAW_SET) {
          // Int / Long / Float / DoubleRawValueBasedInPredicateEvaluator: set.contains(value).  A ScanBasedFilterOperator for the plan (child order,
          // count hooks, statistics all go by the PREDICATE's kind); on the device the leaf is a hash table in LDS -- probed by scan_raw_set_kernel
          // itself when the query has its shape, else by raw_set_bitmap_kernel ahead of the query's kernel, which then reads a kLeafBitmap.
          std::vector<uint64_t> keys;
          pg_status st = check_raw_set(seg, pr, &keys);
          if (st != PG_OK) return st;
          if (keys.empty()) { L.kind = kLeafMatchNone; }
          else {
            const int key_bytes = raw_set_key_bytes(col);
            auto table = std::make_shared<RawSetTable>();
            if (!build_raw_set_table(keys, key_bytes, table.get())) return fail(PG_ERR_UNSUPPORTED, "IN list on raw column %s: no table of %d bytes places its %zu values", col.name.c_str(), kRawSetMaxTableBytes, keys.size());
            lw->raw_set_tables.push_back(table);
            st = ensure_set(ctx, set_idx, table->bytes());
            if (st != PG_OK) return st;
            HIP_TRY(mark_pre_work(ctx));      // (the table is the context's: in pg_execute_batch such a query runs by itself)
            HIP_TRY(hipMemcpyAsync(ctx->d_sets[set_idx], table->words.data(), table->bytes(), hipMemcpyHostToDevice, ctx->stream));
            const uint32_t* d_table = ctx->d_sets[set_idx++];
            if (lw->raw_set_lean_hint) {
              int s = slot_for(lw, seg, pr.column);
              if (s < 0) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
              sp.cols[s].in_filter = 1;
              L.kind = kLeafRawSet; L.col = s; L.set_words = d_table; L.set_bytes = (int32_t)table->bytes(); L.span_hi = (uint32_t)table->bytes();
              L.lo = (int32_t)table->mult; L.span = table->shift; L.lo_hi = key_bytes;
              lw->num_scan_leaves++;
            } else {
              const size_t had = ctx->d_bitmaps.size();
              st = ensure_bitmap(seg, ctx, bitmap_idx);
              if (st != PG_OK) return st;
              // (the context keeps the buffer for its later queries, like its other scratch: part of what pg_segment_device_bytes reports)
              seg->device_bytes += (uint64_t)(ctx->d_bitmaps.size() - had) * (uint64_t)std::max(seg->num_tiles, 1) * kMaxTileSteps * 8;
              unsigned long long* bm = ctx->d_bitmaps[bitmap_idx++];
              RawSetBitmapParams bp;
              memset(&bp, 0, sizeof(bp));
              bp.fwd = col.d_fwd; bp.table = d_table; bp.table_bytes = (uint32_t)table->bytes(); bp.mult = table->mult; bp.shift = table->shift;
              bp.num_docs = seg->num_docs; bp.out = reinterpret_cast<uint32_t*>(bm);
              const int wpb = kBlockThreads / 64;
              // a persistent grid: as many workgroups per CU as registers and the tables (of the 160 KiB of LDS) admit, a tile per wave and round
              const int bpc = std::max(1, std::min(waves_raw_set_bitmap(key_bytes) / wpb, (int)((size_t)(156 * 1024) / (table->bytes() + 256))));
              const long long tiles = ((long long)seg->num_docs + 2047) / 2048;
              launch_raw_set_bitmap(key_bytes, (int)std::max<long long>(1, std::min<long long>((tiles + wpb - 1) / wpb, (long long)seg->num_cus * bpc)), ctx->stream, bp);
              HIP_TRY(hipGetLastError());
              L.kind = kLeafBitmap;
              L.bitmap = bm;
              sp.num_bitmap_leaves++;
            }
          }
        } else if (pr.kind == PG_PRED_RAW_RANGE && col.stored_type == PG_TYPE_LONG) {
          // LongRawValueBasedRangePredicateEvaluator (RangePredicateEvaluatorFactory.java:411-446): inclusive int64 bounds
          if (pr.lo > pr.hi) { L.kind = kLeafMatchNone; }
          else {
            int s = slot_for(lw, seg, pr.column);
            if (s < 0) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
            sp.cols[s].in_filter = 1;
            const uint64_t span = (uint64_t)pr.hi - (uint64_t)pr.lo;
            L.kind = kLeafRawRange64; L.col = s;
            L.lo = (int32_t)(uint32_t)(uint64_t)pr.lo; L.lo_hi = (int32_t)(uint32_t)((uint64_t)pr.lo >> 32);
            L.span = (uint32_t)span; L.span_hi = (uint32_t)(span >> 32);
            lw->num_scan_leaves++;
          }
        } else if (pr.kind == PG_PRED_RAW_RANGE && col.stored_type != PG_TYPE_INT) {
          // Float / DoubleRawValueBasedRangePredicateEvaluator: lo / hi are the bit patterns of the inclusive double bounds.
          // value >= lo && value <= hi  <=>  key(value) in [key(lo'), key(hi')] with a zero lower bound taken as -0.0 and a zero
          // upper bound as +0.0 (primitive compares treat the zeros as equal; NaN values match nothing because their keys lie
          // outside [key(-inf), key(+inf)]).
          double dlo, dhi;
          memcpy(&dlo, &pr.lo, 8); memcpy(&dhi, &pr.hi, 8);
          if (!(dlo <= dhi)) { L.kind = kLeafMatchNone; }
          else {
            int s = slot_for(lw, seg, pr.column);
            if (s < 0) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
            sp.cols[s].in_filter = 1;
            if (dlo == 0.0) dlo = -0.0;
            if (dhi == 0.0) dhi = 0.0;
            auto key = [](double v) { long long bb; memcpy(&bb, &v, 8); return bb ^ ((bb >> 63) & 0x7FFFFFFFFFFFFFFFll); };
            const long long klo = key(dlo), khi = key(dhi);
            const uint64_t span = (uint64_t)khi - (uint64_t)klo;
            L.kind = col.stored_type == PG_TYPE_FLOAT ? kLeafRawRangeF32 : kLeafRawRangeF64; L.col = s;
            L.lo = (int32_t)(uint32_t)(uint64_t)klo; L.lo_hi = (int32_t)(uint32_t)((uint64_t)klo >> 32);
            L.span = (uint32_t)span; L.span_hi = (uint32_t)(span >> 32);
            lw->num_scan_leaves++;
          }
        } else if (pr.kind == PG_PRED_RAW_RANGE) {
          int64_t lo = std::max<int64_t>(pr.lo, std::numeric_limits<int32_t>::min());
          int64_t hi = std::min<int64_t>(pr.hi, std::numeric_limits<int32_t>::max());
          if (lo > hi) { L.kind = kLeafMatchNone; }
          else {
            int s = slot_for(lw, seg, pr.column);
            if (s < 0) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
            sp.cols[s].in_filter = 1;
            L.kind = kLeafRawRange; L.col = s; L.lo = (int32_t)lo; L.span = (uint32_t)(hi - lo);
            lw->num_scan_leaves++;
          }
        } else {
          return fail(PG_ERR_INVALID_ARGUMENT, "unknown predicate kind %d", pr.kind);
        }
      }
      depth++;
    } else if (fn.op == PG_FILTER_NOT) {
      if (depth < 1) return fail(PG_ERR_INVALID_ARGUMENT, "malformed filter tree (NOT without operand)");
    } else if (fn.op == PG_FILTER_AND || fn.op == PG_FILTER_OR) {
      if (fn.num_children < 1 || depth < fn.num_children) return fail(PG_ERR_INVALID_ARGUMENT, "malformed filter tree (node %d)", n);
      depth -= fn.num_children - 1;
    } else {
      return fail(PG_ERR_INVALID_ARGUMENT, "unknown filter op %d", fn.op);
    }
    max_depth = std::max(max_depth, depth);
  }
  if (!seq.empty() && depth != 1) return fail(PG_ERR_INVALID_ARGUMENT, "malformed filter tree (%d roots)", depth);
  if (max_depth > kStackDepth) return fail(PG_ERR_UNSUPPORTED, "filter tree deeper than %d", kStackDepth);
  sp.num_nodes = (int)seq.size();
  // index-driven query: postings first, the scan columns only for tiles the postings did not eliminate
  sp.lazy_columns = (num_bitmap_prefix > 0 && lw->num_scan_leaves > 0 && lazy_node >= 0) ? 1 : 0;
  sp.lazy_node = lazy_node;
  return PG_OK;
}

struct Geometry {
  int blocks = 1;
  int threads = kBlockThreads;
  size_t lds = 0;
  bool table_in_lds = false;
};

constexpr size_t kLdsBudget = 156 * 1024;     // of the 160 KiB per CU; leaves room for the runtime's own use

static long long doc_tiles(const pg_segment* seg) { return ((long long)seg->num_docs + 2047) / 2048; }      // the segment's 2048-doc tiles
// A persistent grid: one workgroup per `per_block` units of work (tiles, or runs of them), at least one, at most `bpc` per CU.
// PINOT_GPU_BLOCKS_PER_CU (g_engine.blocks_per_cu) replaces `bpc` unless the launch is not `overridable`.
static int grid_blocks(const pg_segment* seg, long long units, long long per_block, int bpc, bool overridable = true) {
  if (overridable && g_engine.blocks_per_cu > 0) bpc = g_engine.blocks_per_cu;
  return (int)std::max<long long>(1, std::min<long long>((units + per_block - 1) / per_block, (long long)seg->num_cus * bpc));
}

// Lays out the per-wave LDS region (one staging slot per packed column, 256 bytes per bitmap leaf, the gather queue),
// then picks tile size (32 or 16 steps) and workgroup size so that the most wavefronts stay resident per CU within the
// LDS budget, and sizes the grid to exactly what is co-resident (a persistent grid: a grid larger than residency runs
// in rounds and leaves the chip partly empty during the last one).
// Plan -> kernel parameter block: self-contained node records, statically indexed staging / aggregation descriptors.
void flatten_plan(Lowered* lw) {
  const PlanParams& pl = lw->plan;
  ScanParams& sp = lw->sp;
  sp.num_cols = pl.num_cols;
  sp.num_leaves = pl.num_leaves;
  sp.num_nodes = pl.num_nodes;
  sp.num_agg_cols = pl.num_agg_cols;
  sp.num_bitmap_leaves = 0;
  sp.lazy_columns = pl.lazy_columns;
  sp.lazy_node = pl.lazy_node;
  sp.num_stage = 0;
  for (int c = 0; c < pl.num_cols; ++c) {
    if (pl.cols[c].is_raw) continue;
    DevStage& st = sp.stage[sp.num_stage++];
    st.fwd = pl.cols[c].fwd; st.bits = pl.cols[c].bits; st.slot_off = pl.cols[c].slot_off; st.in_filter = pl.cols[c].in_filter; st.pad = 0;
  }
  for (int n = 0; n < pl.num_nodes; ++n) {
    DevNode& dn = sp.nodes[n];
    memset(&dn, 0, sizeof(dn));
    dn.op = pl.nodes[n].op; dn.flags = pl.nodes[n].flags; dn.num_children = pl.nodes[n].num_children;
    if (pl.nodes[n].op != PG_FILTER_LEAF) continue;
    const DevLeaf& L = pl.leaves[pl.nodes[n].leaf];
    dn.kind = L.kind; dn.exclusive = L.exclusive; dn.lo = L.lo; dn.span = L.span; dn.set_bytes = L.set_bytes; dn.set_words = L.set_words;
    dn.lds_off = L.lds_off;
    if (L.kind == kLeafBitmap) dn.set_words = reinterpret_cast<const uint32_t*>(L.bitmap);   // scan_private_kernel reads the bitmap as dwords
    if (L.kind == kLeafDictRange || L.kind == kLeafDictSet || L.kind == kLeafRawRange || L.kind >= kLeafRawRange64) {
      const DevColumn& c = pl.cols[L.col];
      dn.bits = c.bits; dn.slot_off = c.slot_off; dn.fwd = c.fwd;
    }
    if (L.kind >= kLeafRawRange64) { dn.lo_hi = L.lo_hi; dn.set_bytes = (int32_t)L.span_hi; }
  }
  for (int l = 0; l < pl.num_leaves; ++l) {
    if (pl.leaves[l].kind != kLeafBitmap) continue;
    sp.bitmaps[sp.num_bitmap_leaves] = pl.leaves[l].bitmap;
    sp.bitmap_lds_off[sp.num_bitmap_leaves] = pl.leaves[l].lds_off;
    sp.num_bitmap_leaves++;
  }
  for (int a = 0; a < pl.num_agg_cols; ++a) {
    const DevColumn& c = pl.cols[pl.agg_cols[a].col];
    DevAggCol& ac = sp.agg_cols[a];
    ac.need_sum = pl.agg_cols[a].need_sum; ac.need_minmax = pl.agg_cols[a].need_minmax;
    ac.bits = c.bits; ac.slot_off = c.slot_off; ac.is_raw = c.is_raw; ac.is_plane = c.is_plane; ac.dict_bytes = c.dict_bytes; ac.vkind = c.vkind;
    ac.fwd = c.fwd; ac.dict = c.dict;
  }
}

void finish_geometry(const pg_segment* seg, Lowered* lw, size_t table_bytes, bool need_queue, int max_block_waves, int wave_cap, Geometry* g) {
  ScanParams& sp = lw->sp;
  PlanParams& pl = lw->plan;
  sp.num_docs = seg->num_docs;
  sp.double_buffer = g_engine.double_buffer ? 1 : 0;
  sp.queue_cap = 256;
  const bool table_fits_lds = table_bytes > 0 && table_bytes <= 96 * 1024;
  int best_steps = 32, best_waves = 1, best_resident = -1;
  bool best_table = false;
  for (int steps : {32, 16}) {
    if (g_engine.tile_steps != 0 && steps != g_engine.tile_steps) continue;
    int stage = 0;
    for (int c = 0; c < pl.num_cols; ++c) if (!pl.cols[c].is_raw) stage += ((8 * pl.cols[c].bits * steps + 16) + 15) & ~15;
    stage = std::max(stage, 16);
    const size_t wave_lds = std::max<size_t>((size_t)(sp.double_buffer ? 2 : 1) * stage + 512 * pl.num_bitmap_leaves + (need_queue ? sp.queue_cap * 4 : 0), 128);
    for (int pass = 0; pass < 2; ++pass) {
      const bool in_lds = pass == 0 ? table_fits_lds : false;
      if (pass == 1 && table_fits_lds && best_table) break;     // an LDS-table configuration exists: keep it
      const size_t fixed = in_lds ? table_bytes : 0;
      for (int w = max_block_waves; w >= 1; w >>= 1) {
        const size_t lds_w = (size_t)w * wave_lds + fixed;
        if (lds_w > kLdsBudget) continue;
        const int resident = std::min(wave_cap, (int)(kLdsBudget / lds_w) * w);
        // prefer more resident wavefronts; on ties the larger tile, then the larger workgroup (fewer table copies)
        if (resident > best_resident) { best_resident = resident; best_steps = steps; best_waves = w; best_table = in_lds; }
      }
      if (!table_fits_lds) break;
    }
  }
  if (best_resident < 0) { best_steps = 16; best_waves = 1; best_table = false; }
  // final layout for the chosen tile size
  const int steps = best_steps;
  sp.tile_steps = steps;
  sp.num_tiles = (int)(((long long)seg->num_docs + 64 * steps - 1) / (64 * steps));
  int off = 0;
  for (int c = 0; c < pl.num_cols; ++c) {
    pl.cols[c].slot_off = off;
    if (!pl.cols[c].is_raw) off += ((8 * pl.cols[c].bits * steps + 16) + 15) & ~15;
  }
  sp.stage_bytes = std::max(off, 16);
  off = (sp.double_buffer ? 2 : 1) * sp.stage_bytes;
  sp.bitmap_off = off;
  int boff = 0;
  for (int l = 0; l < pl.num_leaves; ++l) if (pl.leaves[l].kind == kLeafBitmap) { pl.leaves[l].lds_off = boff; boff += 256; }
  sp.bitmap_bytes = boff;
  off += 2 * boff;                            // the posting words of the next tile are always prefetched
  sp.queue_off = off;
  if (need_queue) off += sp.queue_cap * 4;
  sp.wave_lds_bytes = std::max(off, 128);
  g->table_in_lds = best_table;
  g->threads = best_waves * 64;
  g->lds = (size_t)best_waves * sp.wave_lds_bytes + (best_table ? table_bytes : 0);
  g->lds = std::max(g->lds, sizeof(BlockPartial) * (size_t)best_waves + 16);      // the waves' records + the fold flag (publish_block_partial)
  g->blocks = grid_blocks(seg, sp.num_tiles, best_waves, std::max(1, std::min(wave_cap / best_waves, (int)(kLdsBudget / g->lds))));
  flatten_plan(lw);
}

// MIN / MAX key of a column in the 32-bit domain or of any dictionary column (dictId) -> the value as the reference's
// holder sees it ((double) of the typed minimum / maximum).
double agg_value_double(const ColumnDev& col, int32_t key, bool plane) {
  if (col.encoding == PG_FWD_RAW_FIXED_BYTE) return (double)key;
  if (plane) return (double)(col.value_base + col.plane_base + col.plane_scale * (int64_t)key);   // 32-bit planes: base 0, scale 1, key = value
  return col.h_dict_f64[(size_t)key];
}
// Group-by MAX over a FLOAT / DOUBLE dictionary that holds NaN keeps the CPU plan: the group kernels fold dictIds, the NaN entry is the
// largest one, and MaxAggregationFunction.aggregateGroupBySV's `value > holder` never takes a NaN -- the answer is the largest OTHER dictId
// of the group, which a maximum of dictIds has lost once the NaN entry is in.  (Said by pg_query_check and pg_execute alike.)
pg_status fail_group_max_over_nan_dictionary(const char* name) {
  return fail(PG_ERR_UNSUPPORTED, "group-by MAX of dictionary column %s whose dictionary holds NaN (plan-time fallback)", name);
}
// The same for a group's MIN: the smallest dictId of a FLOAT / DOUBLE dictionary is its NaN entry (the last one) only when every value of
// the group is NaN, and `value < holder` never let one in: the holder still has its default.  (MAX over such a dictionary is declined at
// plan time, group_max_over_nan_dictionary: once the NaN dictId has won the fold the group's finite maximum is gone.)
double group_dict_min_double(const ColumnDev& col, int32_t key, bool plane) {
  const double v = agg_value_double(col, key, plane);
  return v != v ? std::numeric_limits<double>::infinity() : v;
}
// An integer sum known exactly (128 bits): sum_i64 is it modulo 2^64, `sum` its correctly rounded double; exact while it
// fits int64 (the reference's double accumulation agrees bit for bit below 2^53 and to rounding above).
void set_integer_sum(pg_agg_value* v, __int128 t) {
  v->sum_i64 = (int64_t)(unsigned long long)(unsigned __int128)t;
  v->sum_exact = ((__int128)v->sum_i64 == t) ? 1 : 0;
  v->sum = (double)t;
}
// what count * base adds back to a sum accumulated in the 32-bit domain
int64_t sum_base(const ColumnDev& col, bool plane) { return col.value_base + (plane ? col.plane_base : 0); }
int64_t sum_scale(const ColumnDev& col, bool plane) { return plane ? col.plane_scale : 1; }
// 64-bit MIN / MAX key of a raw LONG / FLOAT / DOUBLE column (f64_order_key is its own inverse)
double key64_to_double(const ColumnDev& col, long long key) {
  if (col.vkind == kValI64) return (double)key;
  const long long b = key ^ ((key >> 63) & 0x7FFFFFFFFFFFFFFFll);
  double v;
  memcpy(&v, &b, 8);
  return v;
}

// A FLOAT / DOUBLE dictionary is sorted in Double.compare order: a NaN, if the column holds one, is its LAST entry.  MIN / MAX of
// dictionary columns run on dictIds, so both of the reference's NaN rules need this: Math.min / max of the aggregation-only path make
// BOTH extremes NaN once a matching doc has that dictId; the group-by path's `value < holder` / `value > holder` never lets it in.
bool dict_ends_in_nan(const ColumnDev& col) {
  return col.encoding == PG_FWD_FIXED_BIT_DICT && (col.vkind == kValF64 || col.vkind == kValF32) && !col.h_dict_f64.empty() && std::isnan(col.h_dict_f64.back());
}
// MIN / MAX accumulator of a group over a raw FLOAT / DOUBLE column: the order key of the extreme among the group's non-NaN values, or the
// slot's identity when every value was NaN -- the reference's holder then still has its default (Min / MaxAggregationFunction.java:180-186).
double group_key64_to_double(const ColumnDev& col, long long key, bool is_min) {
  if (col.vkind != kValI64 && key == (is_min ? 0x7FFFFFFFFFFFFFFFll : (long long)0x8000000000000000ull))
    return is_min ? std::numeric_limits<double>::infinity() : -std::numeric_limits<double>::infinity();
  return key64_to_double(col, key);
}

inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield" ::: "memory");
#else
  std::this_thread::yield();
#endif
}

// Bounded spin on a pinned sequence number (a query is tens of microseconds to a millisecond of device time: polling beats the
// stream-synchronise wake-up by ~10 us), then the blocking wait: a combine pool may have twice as many such threads as the host has
// cores, none of them may hold a core for longer than its kernel plausibly runs.  `docs`: what the launch scans -- the bound is
// 300 us + 1 ns per 1000 docs (a 1 B-row scan is ~0.6 ms).
template <typename Done>
pg_status wait_polled(hipStream_t stream, long long docs, Done&& done) {
  long long spins = 0;
  std::chrono::steady_clock::time_point until;
  while (!done()) {
    cpu_relax();
    if ((++spins & 0x3FF) != 0) continue;
    const auto now = std::chrono::steady_clock::now();
    if (spins == 0x400) { until = now + std::chrono::nanoseconds(300'000 + docs / 1000); continue; }
    if (now >= until || hipStreamQuery(stream) != hipErrorNotReady) { HIP_TRY(hipStreamSynchronize(stream)); break; }      // finished (or failed) without publishing: the stream's verdict
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return PG_OK;
}

}  // namespace

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

const char* pg_last_error(void) { return g_error.c_str(); }
const char* pg_version(void) { return "pinot_amd 0.1 (gfx950)"; }

pg_status pg_init(const pg_config* config) {
  std::lock_guard<std::mutex> lk(g_engine.mu);
  if (config && config->abi_version != PG_ABI_VERSION) return fail(PG_ERR_INVALID_ARGUMENT, "ABI version mismatch: got %d, built %d", config->abi_version, PG_ABI_VERSION);
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) return fail(PG_ERR_DEVICE, "no HIP device available: %s", hipGetErrorString(e));
  g_engine.physical_devices = count;
  const char* ald = getenv("PINOT_GPU_ALIAS_DEVICES");
  g_engine.logical_devices = (ald && atoi(ald) > count) ? std::min(atoi(ald), 64) : count;
  int dev = config ? config->device_id : 0;
  if (dev < 0 || dev >= g_engine.logical_devices) return fail(PG_ERR_INVALID_ARGUMENT, "device %d out of range (have %d)", dev, g_engine.logical_devices);
  g_engine.device = dev;
  g_engine.blocks_per_cu = config ? config->blocks_per_cu : 0;
  g_engine.flags = config ? config->flags : 0;
  const char* nodma = getenv("PINOT_GPU_NO_DMA");
  g_engine.use_dma = !(nodma && nodma[0] == '1');
  const char* vp = getenv("PINOT_GPU_VALUE_PLANE");
  g_engine.value_plane = vp ? atoi(vp) : -1;
  const char* db = getenv("PINOT_GPU_DOUBLE_BUFFER");
  g_engine.double_buffer = db && db[0] == '1';
  const char* drv = getenv("PINOT_GPU_DIRECT_RESULT");
  g_engine.direct_result = !(drv && drv[0] == '0');
  const char* ffz = getenv("PINOT_GPU_FOLD_FINALIZE");
  g_engine.fold_finalize = ffz ? (ffz[0] == '0' ? 0 : 1) : -1;
  const char* foc = getenv("PINOT_GPU_FOLD_ONE_COUNTER");
  g_engine.fold_one_counter = foc ? (foc[0] == '0' ? 0 : 1) : 1;
  const char* prs = getenv("PINOT_GPU_POLL_RESULT");
  g_engine.poll_result = !(prs && prs[0] == '0');
  const char* lsk = getenv("PINOT_GPU_LANE_SKIP");
  g_engine.lane_skip = !(lsk && lsk[0] == '0');
  const char* bbc = getenv("PINOT_GPU_BATCH_BLOCKS_PER_CU");
  g_engine.batch_blocks_per_cu_forced = bbc != nullptr;
  g_engine.batch_blocks_per_cu = (bbc && atoi(bbc) > 0) ? atoi(bbc) : 4;      // measured on 64 x 10 M rows: 2 / 4 / 8 / 16 / 32 / 64 -> 0.77 / 0.55 / 0.57 / 0.59 / 0.61 / 0.65 ms
  const char* ssp = getenv("PINOT_GPU_SCAN_SPARSE");
  g_engine.scan_sparse = !(ssp && ssp[0] == '0');
  const char* ssm = getenv("PINOT_GPU_SCAN_SIMPLE");
  g_engine.scan_simple = !(ssm && ssm[0] == '0');
  const char* ssv = getenv("PINOT_GPU_SCAN_SIMPLE_VALID");
  g_engine.scan_simple_valid = ssv ? (ssv[0] == '0' ? 0 : (ssv[0] == '2' ? 2 : 1)) : 1;
  const char* spp = getenv("PINOT_GPU_SCAN_SIMPLE_PIPE");
  g_engine.scan_simple_pipe = spp ? (spp[0] == '0' ? 0 : (spp[0] == '2' ? 2 : 1)) : 1;
  const char* sdm = getenv("PINOT_GPU_SCAN_SIMPLE_DMA");
  g_engine.scan_simple_dma = sdm ? (sdm[0] == '0' ? 0 : (sdm[0] == '2' ? 2 : 1)) : 1;
  const char* sdp = getenv("PINOT_GPU_SCAN_SIMPLE_DMA_PAIR");
  g_engine.dma_pair = sdp && sdp[0] == '0' ? 0 : 1;
  const char* sdn = getenv("PINOT_GPU_SCAN_SIMPLE_DMA_NT");
  g_engine.dma_nt = sdn ? (sdn[0] == '0' ? 0 : 1) : -1;
  const char* sdb = getenv("PINOT_GPU_SCAN_SIMPLE_DMA_BLOCKS_PER_CU");
  g_engine.dma_blocks_per_cu = sdb && atoi(sdb) > 0 ? atoi(sdb) : 0;
  const char* srw = getenv("PINOT_GPU_SCAN_RAW");
  g_engine.scan_raw = !(srw && srw[0] == '0');
  const char* srs = getenv("PINOT_GPU_SCAN_RAW_SET");
  g_engine.scan_raw_set = !(srs && srs[0] == '0');
  const char* bla = getenv("PINOT_GPU_BATCH_LAUNCH");
  g_engine.batch_launch = !(bla && bla[0] == '0');
  auto env_on = [](const char* name) { const char* v = getenv(name); return !(v && v[0] == '0'); };
  g_engine.lean_batch = env_on("PINOT_GPU_LEAN_BATCH");
  g_engine.set_lds = env_on("PINOT_GPU_SET_LDS");
  g_engine.distinct_lds = env_on("PINOT_GPU_DISTINCT_LDS");
  g_engine.percentile_lds = env_on("PINOT_GPU_PERCENTILE_LDS");
  { const char* cv = getenv("PINOT_GPU_COLLECT"); g_engine.collect = cv != nullptr && cv[0] == '1'; }
  { const char* cd = getenv("PINOT_GPU_CHUNK_DECODE"); g_engine.chunk_decode_host = cd != nullptr && strcmp(cd, "host") == 0; }
  g_engine.partition_two_level = env_on("PINOT_GPU_PARTITION_TWO_LEVEL");
  g_engine.fsm_perm = env_on("PINOT_GPU_FSM_PERM");
  g_engine.fsm_stats = env_on("PINOT_GPU_FSM_STATS");
  g_engine.fsm_fused = env_on("PINOT_GPU_FSM_FUSED");
  g_engine.fsm_episodes = env_on("PINOT_GPU_FSM_EPISODES");
  g_engine.index_gather = env_on("PINOT_GPU_INDEX_GATHER");
  g_engine.batch_index = env_on("PINOT_GPU_BATCH_INDEX");
  { const char* iaw = getenv("PINOT_GPU_INDEX_AND_WAVES"); g_engine.index_and_waves = iaw ? std::max(-64, std::min(32, atoi(iaw))) : 0; }
  g_engine.group_one_launch = env_on("PINOT_GPU_GROUP_ONE_LAUNCH");
  g_engine.plan_cache = env_on("PINOT_GPU_PLAN_CACHE");
  g_engine.group_publish = env_on("PINOT_GPU_GROUP_PUBLISH");
  const char* bmo = getenv("PINOT_GPU_BATCH_MORE");
  g_engine.batch_more = !(bmo && bmo[0] == '0');
  const char* bgr = getenv("PINOT_GPU_BATCH_GROUP");
  g_engine.batch_group = !(bgr && bgr[0] == '0');
  const char* bhi = getenv("PINOT_GPU_BATCH_HIST");
  g_engine.batch_hist = !(bhi && bhi[0] == '0');
  const char* lp2 = getenv("PINOT_GPU_LEAP2");
  g_engine.leap2 = !(lp2 && lp2[0] == '0');
  const char* spl = getenv("PINOT_GPU_SPARSE_LANES");
  g_engine.sparse_lanes = spl ? std::max(0, std::min(64, atoi(spl))) : 32;
  const char* pgv = getenv("PINOT_GPU_PLANE_GCD");
  g_engine.plane_gcd = !(pgv && pgv[0] == '0');
  const char* spv = getenv("PINOT_GPU_SCAN_PRIVATE");
  g_engine.scan_private = !(spv && spv[0] == '0');
  const char* gpv = getenv("PINOT_GPU_GROUP_PRIVATE");
  g_engine.group_private = !(gpv && gpv[0] == '0');
  const char* grv = getenv("PINOT_GPU_GROUP_REPLICAS");
  g_engine.group_log_replicas = grv ? std::max(0, std::min(4, atoi(grv))) : 3;
  const char* stp = getenv("PINOT_GPU_SCAN_TYPED_PRIVATE");
  g_engine.scan_typed_private = !(stp && stp[0] == '0');
  const char* gpt = getenv("PINOT_GPU_GROUP_PARTITION");
  g_engine.group_partition = !(gpt && gpt[0] == '0');
  g_engine.partition_min_docs = (gpt && gpt[0] == 'f') ? 0 : (1ll << 22);
  const char* sns = getenv("PINOT_GPU_SCAN_NARROW_SINGLE");
  g_engine.scan_narrow_single = !(sns && sns[0] == '0');
  const char* snw = getenv("PINOT_GPU_SCAN_NARROW");
  g_engine.scan_narrow = !(snw && snw[0] == '0');
  const char* gtb = getenv("PINOT_GPU_GROUP_TABLE_BYTES");
  g_engine.group_table_bytes = (gtb && atoll(gtb) > 0) ? (unsigned long long)atoll(gtb) : (64ull << 30);
  const char* gpk = getenv("PINOT_GPU_GROUP_PACK");
  g_engine.group_pack = !(gpk && gpk[0] == '0');
  const char* gw = getenv("PINOT_GPU_GROUP_WAVES");
  g_engine.group_waves = (gw && atoi(gw) > 0) ? atoi(gw) : 0;
  const char* hs = getenv("PINOT_GPU_HIST");
  g_engine.hist = hs ? atoi(hs) : -1;
  const char* hbl = getenv("PINOT_GPU_HIST_BLOCKS");
  g_engine.hist_blocks = (hbl && atoi(hbl) > 0) ? atoi(hbl) : 0;
  const char* hg = getenv("PINOT_GPU_HIST_GUARD");
  g_engine.hist_guard = hg && hg[0] == '1';
  const char* hb = getenv("PINOT_GPU_HIST_BITS");
  g_engine.hist_bits = (hb && (atoi(hb) == 8 || atoi(hb) == 16)) ? atoi(hb) : 0;
  const char* ts = getenv("PINOT_GPU_TILE_STEPS");
  g_engine.tile_steps = (ts && (atoi(ts) == 16 || atoi(ts) == 32)) ? atoi(ts) : 0;
  // (pg_init may be called again with another environment -- tools/ab_r3.py, tests: every switch goes back to its default first)
  g_engine.raw64_coalesced = true; g_engine.wide_plane = -1; g_engine.partition_stats_cache = true; g_engine.partition_packed = true;
  g_engine.plane_async = true; g_engine.staged_h2d = true; g_engine.exact_stats_docs = 64ll << 20;
  const char* r64 = getenv("PINOT_GPU_RAW64_COALESCED");
  if (r64) g_engine.raw64_coalesced = atoi(r64) != 0;
  const char* wpl = getenv("PINOT_GPU_WIDE_PLANE");
  if (wpl) g_engine.wide_plane = atoi(wpl);
  const char* psc = getenv("PINOT_GPU_PARTITION_STATS_CACHE");
  if (psc) g_engine.partition_stats_cache = atoi(psc) != 0;
  const char* ppk = getenv("PINOT_GPU_PARTITION_PACKED");
  if (ppk) g_engine.partition_packed = atoi(ppk) != 0;
  const char* pas = getenv("PINOT_GPU_PLANE_ASYNC");
  if (pas) g_engine.plane_async = atoi(pas) != 0;
  const char* sh2d = getenv("PINOT_GPU_STAGED_H2D");
  if (sh2d) g_engine.staged_h2d = atoi(sh2d) != 0;
  {
    // value-plane budget: pg_config, then the environment; default a quarter of the device's memory
    uint64_t budget = config ? config->plane_budget_bytes : 0;
    const char* pb = getenv("PINOT_GPU_PLANE_BUDGET_BYTES");
    if (pb) budget = strtoull(pb, nullptr, 10);
    if (budget == 0) {
      size_t free_bytes = 0, total_bytes = 0;
      (void)hipSetDevice(phys_device(dev));
      if (hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess) budget = total_bytes / 4; else budget = 64ull << 30;
    }
    std::lock_guard<std::mutex> lk(g_planes.mu);
    g_planes.budget_bytes = budget;
  }
  const char* esd = getenv("PINOT_GPU_EXACT_FILTER_STATS_DOCS");
  if (esd) g_engine.exact_stats_docs = atoll(esd);
  const char* bpc = getenv("PINOT_GPU_BLOCKS_PER_CU");
  if (bpc && atoi(bpc) > 0) g_engine.blocks_per_cu = atoi(bpc);
  g_engine.epoch.fetch_add(1, std::memory_order_release);      // (what segments remember of earlier lowerings was made under the previous settings)
  g_engine.initialized = true;
  return PG_OK;
}

pg_status pg_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_engine.mu);
  g_engine.initialized = false;
  { std::lock_guard<std::mutex> sl(g_stage.mu); destroy_stage_pool_locked(); }
  return PG_OK;
}

pg_status pg_device_info(int32_t device_id, char* arch_name, int32_t arch_name_len, int32_t* num_cus, uint64_t* hbm_bytes) {
  if (!device_id_ok(device_id)) return fail(PG_ERR_INVALID_ARGUMENT, "device id %d out of range", device_id);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, phys_device(device_id)));
  if (arch_name && arch_name_len > 0) { strncpy(arch_name, prop.gcnArchName, (size_t)arch_name_len - 1); arch_name[arch_name_len - 1] = 0; }
  if (num_cus) *num_cus = prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
  return PG_OK;
}

pg_status pg_device_count(int32_t* out_devices, int32_t* out_physical) {
  if (!g_engine.initialized) return fail(PG_ERR_NOT_INITIALIZED, "pg_init has not been called");
  if (out_devices) *out_devices = g_engine.logical_devices;
  if (out_physical) *out_physical = g_engine.physical_devices;
  return PG_OK;
}

pg_status pg_measure_stream_read(int32_t device_id, uint64_t bytes, int32_t launches, double* out_gbps) {
  if (!out_gbps || bytes < (1u << 20) || launches < 1) return fail(PG_ERR_INVALID_ARGUMENT, "bad stream probe arguments");
  if (!device_id_ok(device_id)) return fail(PG_ERR_INVALID_ARGUMENT, "device id %d out of range", device_id);
  HIP_TRY(hipSetDevice(phys_device(device_id)));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, phys_device(device_id)));
  uint8_t* buf = nullptr;
  unsigned long long* sink = nullptr;
  HIP_TRY(hipMalloc((void**)&buf, bytes));
  hipError_t e = hipMalloc((void**)&sink, 8);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (e == hipSuccess) e = hipMemset(buf, 0, bytes);
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  float best = 0.f;
  if (e == hipSuccess) {
    const unsigned blocks = (unsigned)prop.multiProcessorCount * 8u;        // 2048 threads per CU: a persistent grid, like the scan kernels
    for (int i = 0; i < launches + 2 && e == hipSuccess; ++i) {
      (void)hipEventRecord(e0, 0);
      stream_read_probe_kernel<<<dim3(blocks), dim3(kBlockThreads), 0, 0>>>(reinterpret_cast<const uint4*>(buf), (size_t)(bytes / 16), sink);
      (void)hipEventRecord(e1, 0);
      e = hipEventSynchronize(e1);
      float ms = 0.f;
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
      if (i >= 2 && ms > 0.f) best = std::max(best, (float)((double)bytes / (ms * 1e-3) / 1e9));
    }
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(buf);
  if (sink) (void)hipFree(sink);
  if (e != hipSuccess) return fail(PG_ERR_DEVICE, "stream probe: %s", hipGetErrorString(e));
  *out_gbps = best;
  return PG_OK;
}

// The chunks of an LZ4 / SNAPPY raw forward index (validated: pgcodec::validate_chunk_table) -> `d_values`, the column's dense value area.
// On the device: the file is uploaded as it is, chunk_decode_kernel decodes every chunk (pg_chunk_decode.h), and the compressed copy is freed
// before this returns.  Chunks above PG_CHUNK_DECODE_MAX_BYTES (a hand-set targetDocsPerChunk) and everything under PINOT_GPU_CHUNK_DECODE=host
// take the host decoder of pg_chunk_codec.h and are uploaded as values.
static pg_status decode_raw_chunks(const pg_segment* seg, const ColumnDev& col, const pgcodec::ChunkFile& cf, const uint8_t* file, uint64_t file_size, uint8_t* d_values) {
  const uint64_t chunk_bytes = (uint64_t)cf.docs_per_chunk * (uint64_t)cf.entry_size;
  const uint64_t value_area = (uint64_t)seg->num_docs * (uint64_t)cf.entry_size;
  auto malformed = [&](int chunk, int code) {
    return fail(PG_ERR_INVALID_ARGUMENT, "column %s: chunk %d of %d is not a well-formed %s chunk (error %d)", col.name.c_str(), chunk, cf.num_chunks, pgcodec::codec_name(cf.codec), code);
  };
  if (g_engine.chunk_decode_host || chunk_bytes > PG_CHUNK_DECODE_MAX_BYTES) {
    std::vector<uint8_t> values((size_t)value_area);
    int bad = 0;
    const int r = pgcodec::decode_file_host(cf, file, file_size, seg->num_docs, values.data(), &bad);
    if (r != pgcodec::kEnd) return malformed(bad, r);
    const hipError_t e = h2d_copy(d_values, values.data(), values.size(), phys_device(seg->device));
    if (e != hipSuccess) return fail(PG_ERR_DEVICE, "column %s: H2D copy: %s", col.name.c_str(), hipGetErrorString(e));
    return PG_OK;
  }
  const size_t status_at = ((size_t)file_size + 8 + 7) / 8 * 8;      // (8 readable bytes behind the file, then the status word)
  uint8_t* d_file = nullptr;
  hipError_t e = hipMalloc((void**)&d_file, status_at + 8);
  if (e != hipSuccess) return fail(PG_ERR_OUT_OF_MEMORY, "column %s: hipMalloc(%zu) for the compressed chunks: %s", col.name.c_str(), status_at + 8, hipGetErrorString(e));
  unsigned long long status = ~0ull;
  e = hipMemset(d_file + file_size, 0, status_at - (size_t)file_size);
  if (e == hipSuccess) e = hipMemcpy(d_file + status_at, &status, 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = h2d_copy(d_file, file, (size_t)file_size, phys_device(seg->device));
  if (e == hipSuccess) {
    ChunkDecodeParams p;
    p.file = d_file; p.file_size = file_size; p.header_start = cf.header_start; p.offset_bytes = cf.offset_bytes; p.num_chunks = cf.num_chunks;
    p.chunk_bytes = (unsigned int)chunk_bytes;
    p.last_chunk_bytes = (unsigned int)pgcodec::chunk_expect_bytes(cf, seg->num_docs, cf.num_chunks - 1);
    p.lds_stride = (unsigned int)((chunk_bytes + 15) / 16 * 16);
    p.out = d_values;
    p.status = reinterpret_cast<unsigned long long*>(d_file + status_at);
    // as many chunks per workgroup as fit 64 KiB of LDS (at most four), as many workgroups per CU as fit its 160 KiB (at most eight)
    const int waves = (int)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)kChunkDecodeMaxWaves, (uint64_t)PG_CHUNK_DECODE_MAX_BYTES / p.lds_stride, (uint64_t)cf.num_chunks}));
    const int per_cu = (int)std::max<uint64_t>(1, std::min<uint64_t>(8, (160u * 1024u) / ((uint64_t)waves * p.lds_stride)));
    const int blocks = (int)std::min<long long>(((long long)cf.num_chunks + waves - 1) / waves, (long long)seg->num_cus * per_cu);
    launch_chunk_decode(cf.codec, blocks, waves, 0, p);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(&status, d_file + status_at, 8, hipMemcpyDeviceToHost);      // (waits for the kernel)
  }
  (void)hipFree(d_file);
  if (e != hipSuccess) return fail(PG_ERR_DEVICE, "column %s: chunk decode: %s", col.name.c_str(), hipGetErrorString(e));
  if (status != ~0ull) return malformed((int)(status >> 8), (int)(status & 255));
  return PG_OK;
}

pg_status pg_segment_open(const pg_segment_desc* desc, pg_segment** out_segment) {
  if (!g_engine.initialized) return fail(PG_ERR_NOT_INITIALIZED, "pg_init has not been called");
  if (!desc || !out_segment) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  if (desc->num_docs < 0 || desc->num_columns < 0 || (desc->num_columns > 0 && !desc->columns)) return fail(PG_ERR_INVALID_ARGUMENT, "bad segment descriptor");
  pg_segment* seg = new pg_segment();
  seg->device = desc->device_id >= 0 ? desc->device_id : g_engine.device;
  if (seg->device >= g_engine.logical_devices) { const int d = seg->device; delete seg; return fail(PG_ERR_INVALID_ARGUMENT, "pg_segment_desc.device_id %d out of range (have %d)", d, g_engine.logical_devices); }
  seg->num_docs = desc->num_docs;
  seg->num_tiles = (int)(((long long)desc->num_docs + kMaxTileDocs - 1) / kMaxTileDocs);   // 2048-doc tiles (buffer padding unit)
  seg->name = desc->name ? desc->name : "";
  pg_status st = PG_OK;
  auto bail = [&](pg_status s) { free_segment(seg); return s; };
  {
    hipError_t e = hipSetDevice(phys_device(seg->device));
    if (e != hipSuccess) return bail(fail(PG_ERR_DEVICE, "hipSetDevice(%d): %s", seg->device, hipGetErrorString(e)));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, phys_device(seg->device));
    if (e != hipSuccess) return bail(fail(PG_ERR_DEVICE, "hipGetDeviceProperties: %s", hipGetErrorString(e)));
    seg->num_cus = prop.multiProcessorCount;
    // Test switch: every grid of this segment is sized as if the device had this many CUs.  With 1, a 100 000-doc segment is ~50 tiles for
    // ~32 waves -- every kernel's tile loop runs more than once per wave on the suite's SMALL segments (a kernel that was
    // wrong from a wave's second tile on passed every test below 4.5 M docs on the full grid).
    const char* tc = getenv("PINOT_GPU_TEST_CUS");
    if (tc && atoi(tc) > 0) seg->num_cus = atoi(tc);
  }
  seg->cols.resize((size_t)desc->num_columns);
  for (int i = 0; i < desc->num_columns; ++i) {
    const pg_column_desc& cd = desc->columns[i];
    ColumnDev& col = seg->cols[(size_t)i];
    col.name = cd.name ? cd.name : "";
    col.stored_type = cd.stored_type;
    col.encoding = cd.fwd_encoding;
    col.bits = cd.bits_per_value;
    col.cardinality = cd.cardinality;
    if (cd.stored_type < PG_TYPE_INT || cd.stored_type > PG_TYPE_DOUBLE) return bail(fail(PG_ERR_UNSUPPORTED, "column %s: stored type %d is not offloaded", col.name.c_str(), cd.stored_type));
    const int value_bytes = (cd.stored_type == PG_TYPE_INT || cd.stored_type == PG_TYPE_FLOAT) ? 4 : 8;
    if (!cd.fwd_data && desc->num_docs > 0) return bail(fail(PG_ERR_INVALID_ARGUMENT, "column %s: missing forward index", col.name.c_str()));
    const uint8_t* fwd = (const uint8_t*)cd.fwd_data;
    if (cd.fwd_encoding == PG_FWD_FIXED_BIT_DICT) {
      if (cd.bits_per_value < 1 || cd.bits_per_value > 31) return bail(fail(PG_ERR_INVALID_ARGUMENT, "column %s: bits_per_value %d", col.name.c_str(), cd.bits_per_value));
      // FixedBitIntReaderWriter precondition (segl/io/util/FixedBitIntReaderWriter.java:30-33), in 64-bit
      const uint64_t expect = ((uint64_t)desc->num_docs * (uint64_t)cd.bits_per_value + 7) / 8;
      if (cd.fwd_size != expect) return bail(fail(PG_ERR_INVALID_ARGUMENT, "column %s: forward index is %llu bytes, expected %llu", col.name.c_str(), (unsigned long long)cd.fwd_size, (unsigned long long)expect));
      // BaseImmutableDictionary precondition (BaseImmutableDictionary.java:51-53)
      if (cd.cardinality < 1 || !cd.dict_data || cd.dict_size != (uint64_t)cd.cardinality * (uint64_t)value_bytes) return bail(fail(PG_ERR_INVALID_ARGUMENT, "column %s: dictionary buffer size mismatch", col.name.c_str()));
      col.fwd_alloc_bytes = (size_t)std::max(seg->num_tiles, 1) * 256 * (size_t)cd.bits_per_value + 64;
      hipError_t e = hipMalloc((void**)&col.d_fwd_alloc, col.fwd_alloc_bytes);
      if (e != hipSuccess) return bail(fail(PG_ERR_OUT_OF_MEMORY, "column %s: hipMalloc(%zu): %s", col.name.c_str(), col.fwd_alloc_bytes, hipGetErrorString(e)));
      col.d_fwd = col.d_fwd_alloc;
      // zero the padding past the file bytes so tail tiles decode deterministic (masked) values
      size_t tail = col.fwd_alloc_bytes - (size_t)cd.fwd_size;
      e = hipMemset(col.d_fwd_alloc + cd.fwd_size, 0, tail);
      if (e == hipSuccess && cd.fwd_size) e = h2d_copy(col.d_fwd_alloc, fwd, (size_t)cd.fwd_size, phys_device(seg->device));
      if (e != hipSuccess) return bail(fail(PG_ERR_DEVICE, "column %s: H2D copy: %s", col.name.c_str(), hipGetErrorString(e)));
      // Dictionary values -> host order (IntDictionary / LongDictionary / FloatDictionary / DoubleDictionary: C big-endian
      // fixed-width values, ascending; FixedByteValueReaderWriter.getInt/getLong/getFloat/getDouble)
      const size_t C = (size_t)cd.cardinality;
      const uint8_t* dp = (const uint8_t*)cd.dict_data;
      col.h_dict_f64.resize(C);
      std::vector<unsigned long long> wide;
      if (cd.stored_type == PG_TYPE_INT) {
        col.h_dict.resize(C); col.h_dict_i64.resize(C);
        for (size_t d = 0; d < C; ++d) { col.h_dict[d] = (int32_t)be32(dp + 4 * d); col.h_dict_i64[d] = col.h_dict[d]; col.h_dict_f64[d] = (double)col.h_dict[d]; }
      } else if (cd.stored_type == PG_TYPE_LONG) {
        col.h_dict_i64.resize(C);
        for (size_t d = 0; d < C; ++d) {
          col.h_dict_i64[d] = (int64_t)(((uint64_t)be32(dp + 8 * d) << 32) | (uint64_t)be32(dp + 8 * d + 4));
          col.h_dict_f64[d] = (double)col.h_dict_i64[d];
        }
        const uint64_t range = (uint64_t)col.h_dict_i64[C - 1] - (uint64_t)col.h_dict_i64[0];
        if (col.h_dict_i64[C - 1] >= col.h_dict_i64[0] && range < (1ull << 31)) {
          // offset dictionary: the whole 32-bit machinery applies to (value - min)
          col.value_base = col.h_dict_i64[0];
          col.h_dict.resize(C);
          for (size_t d = 0; d < C; ++d) col.h_dict[d] = (int32_t)(col.h_dict_i64[d] - col.value_base);
        } else {
          col.vkind = kValI64;
          wide.resize(C);
          for (size_t d = 0; d < C; ++d) wide[d] = (unsigned long long)col.h_dict_i64[d];
        }
      } else {
        col.vkind = kValF64;
        wide.resize(C);
        for (size_t d = 0; d < C; ++d) {
          double v;
          if (cd.stored_type == PG_TYPE_FLOAT) { const uint32_t b = be32(dp + 4 * d); float f; memcpy(&f, &b, 4); v = (double)f; }
          else { const uint64_t b = ((uint64_t)be32(dp + 8 * d) << 32) | (uint64_t)be32(dp + 8 * d + 4); memcpy(&v, &b, 8); }
          col.h_dict_f64[d] = v;
          memcpy(&wide[d], &v, 8);
        }
      }
      if (col.vkind == kValI32) {
        const PlaneShape ps = compute_plane_shape(col);
        col.shape_base = ps.base; col.shape_scale = ps.scale; col.shape_bits = ps.bits; col.shape_is_fwd = ps.is_fwd;
        e = hipMalloc((void**)&col.d_dict, C * 4);
        if (e == hipSuccess) e = hipMemcpy(col.d_dict, col.h_dict.data(), C * 4, hipMemcpyHostToDevice);
      } else {
        e = hipMalloc((void**)&col.d_dict64, C * 8);
        if (e == hipSuccess) e = hipMemcpy(col.d_dict64, wide.data(), C * 8, hipMemcpyHostToDevice);
      }
      if (e != hipSuccess) return bail(fail(PG_ERR_DEVICE, "column %s: dictionary upload: %s", col.name.c_str(), hipGetErrorString(e)));
      seg->device_bytes += col.fwd_alloc_bytes + C * (col.vkind == kValI32 ? 4 : 8);
    } else if (cd.fwd_encoding == PG_FWD_RAW_FIXED_BYTE) {
      // BaseChunkForwardIndexReader header (BaseChunkForwardIndexReader.java:61-111; pg_chunk_codec.h)
      if (cd.fwd_size < 16) return bail(fail(PG_ERR_INVALID_ARGUMENT, "column %s: raw forward index too small", col.name.c_str()));
      if ((int)be32(fwd) > 1 && cd.fwd_size < 28) return bail(fail(PG_ERR_INVALID_ARGUMENT, "column %s: raw forward index header truncated", col.name.c_str()));
      pgcodec::ChunkFile cf;
      if (pgcodec::parse_chunk_header(fwd, cd.fwd_size, &cf) != pgcodec::kFileOk)
        return bail(fail(PG_ERR_INVALID_ARGUMENT, "column %s: raw forward index header holds a negative count", col.name.c_str()));
      const int compression = cf.codec;
      // LZ4 and SNAPPY chunks are decoded below, once, into the value area a PASS_THROUGH file has.  ZSTANDARD and GZIP need an entropy decoder;
      // the fixed-byte writers never produce LZ4_LENGTH_PREFIXED.
      if (compression != pgcodec::kPassThrough && compression != pgcodec::kLz4 && compression != pgcodec::kSnappy)
        return bail(fail(PG_ERR_UNSUPPORTED, "column %s: %s raw chunks are not offloaded (compressionType=%d): only PASS_THROUGH, LZ4 and SNAPPY are", col.name.c_str(), pgcodec::codec_name(compression), compression));
      const bool compressed = compression != pgcodec::kPassThrough;
      const int entry_size = cf.entry_size;
      if (entry_size != value_bytes) return bail(fail(PG_ERR_UNSUPPORTED, "column %s: raw entry size %d for stored type %d", col.name.c_str(), entry_size, cd.stored_type));
      col.vkind = cd.stored_type == PG_TYPE_INT ? kValI32 : (cd.stored_type == PG_TYPE_LONG ? kValI64 : (cd.stored_type == PG_TYPE_FLOAT ? kValF32 : kValF64));
      const uint64_t raw_start = cf.data_start;
      const uint64_t value_area = (uint64_t)desc->num_docs * (uint64_t)value_bytes;
      if (!compressed && raw_start + value_area > cd.fwd_size) return bail(fail(PG_ERR_INVALID_ARGUMENT, "column %s: raw forward index shorter than numDocs", col.name.c_str()));
      if (compressed && desc->num_docs > 0) {
        // header and offset table, before anything touches the device
        const int vs = pgcodec::validate_chunk_table(cf, fwd, cd.fwd_size, desc->num_docs);
        if (vs != pgcodec::kFileOk)
          return bail(fail(PG_ERR_INVALID_ARGUMENT, "column %s: %s raw forward index: %s", col.name.c_str(), pgcodec::codec_name(compression),
                           vs == pgcodec::kFileBadOffsets ? "chunk offsets decrease or point outside the file"
                           : vs == pgcodec::kFileBadChunkCount ? "numChunks does not match numDocs and numDocsPerChunk"
                           : vs == pgcodec::kFileTruncated ? "the chunk offset table does not lie inside the file" : "the header is not one of versions 1 to 4 with positive sizes"));
      }
      // The resident image of a compressed column is its PASS_THROUGH twin's: the same header and offset table sizes, then the dense values.
      const uint64_t image_size = compressed ? raw_start + value_area : cd.fwd_size;
      // padded so that whole 2048-doc tiles can be read past numDocs (the lane-private kernels never clamp docIds)
      // The file is placed so that the VALUES (not the header) start on a 256-byte boundary: a lane's 32 docs are then whole,
      // aligned 16-byte loads and a tile's rows whole cache lines (the header is 28 + 4 * numChunks bytes: any multiple of 4).
      const size_t lead = (256 - (size_t)(raw_start % 256)) % 256;
      col.fwd_alloc_bytes = lead + std::max<size_t>((size_t)image_size, (size_t)raw_start + (size_t)std::max(seg->num_tiles, 1) * 2048 * (size_t)value_bytes) + 64;
      hipError_t e = hipMalloc((void**)&col.d_fwd_alloc, col.fwd_alloc_bytes);
      if (e != hipSuccess) return bail(fail(PG_ERR_OUT_OF_MEMORY, "column %s: hipMalloc(%zu): %s", col.name.c_str(), col.fwd_alloc_bytes, hipGetErrorString(e)));
      e = hipMemset(col.d_fwd_alloc, 0, col.fwd_alloc_bytes);
      if (e == hipSuccess && !compressed) e = h2d_copy(col.d_fwd_alloc + lead, fwd, (size_t)cd.fwd_size, phys_device(seg->device));
      if (e != hipSuccess) return bail(fail(PG_ERR_DEVICE, "column %s: H2D copy: %s", col.name.c_str(), hipGetErrorString(e)));
      if (compressed && desc->num_docs > 0) {
        const pg_status dst = decode_raw_chunks(seg, col, cf, fwd, cd.fwd_size, col.d_fwd_alloc + lead + raw_start);
        if (dst != PG_OK) return bail(dst);
      }
      col.d_fwd = col.d_fwd_alloc + lead + raw_start;
      col.bits = 32;
      col.cardinality = 0;
      seg->device_bytes += col.fwd_alloc_bytes;
    } else {
      return bail(fail(PG_ERR_UNSUPPORTED, "column %s: unknown forward-index encoding %d", col.name.c_str(), cd.fwd_encoding));
    }
    if (cd.inv_data && cd.inv_size && cd.fwd_encoding == PG_FWD_FIXED_BIT_DICT) {
      // BitmapInvertedIndexReader (BitmapInvertedIndexReader.java:45-62)
      const uint8_t* inv = (const uint8_t*)cd.inv_data;
      const uint64_t offsets_end = ((uint64_t)cd.cardinality + 1) * 4;
      if (cd.inv_size < offsets_end) return bail(fail(PG_ERR_INVALID_ARGUMENT, "column %s: inverted index too small", col.name.c_str()));
      const uint64_t first_offset = be32(inv);
      col.posting_first.assign((size_t)cd.cardinality + 1, 0);
      for (int d = 0; d < cd.cardinality; ++d) {
        col.posting_first[(size_t)d] = (int64_t)col.h_dir.size();
        const uint64_t o0 = be32(inv + 4 * (size_t)d), o1 = be32(inv + 4 * (size_t)(d + 1));
        if (o1 < o0 || offsets_end + (o1 - first_offset) > cd.inv_size) return bail(fail(PG_ERR_INVALID_ARGUMENT, "column %s: inverted index offsets out of range", col.name.c_str()));
        st = parse_roaring(inv, offsets_end + (o0 - first_offset), o1 - o0, &col.h_dir);
        if (st != PG_OK) return bail(st);
      }
      col.posting_first[(size_t)cd.cardinality] = (int64_t)col.h_dir.size();
      col.posting_docs.assign((size_t)cd.cardinality, 0);
      for (int d = 0; d < cd.cardinality; ++d)
        for (int64_t k = col.posting_first[(size_t)d]; k < col.posting_first[(size_t)d + 1]; ++k) col.posting_docs[(size_t)d] += (int64_t)col.h_dir[(size_t)k].cardinality;
      hipError_t e = hipMalloc((void**)&col.d_inv, (size_t)cd.inv_size + 64);
      if (e == hipSuccess) e = h2d_copy(col.d_inv, inv, (size_t)cd.inv_size, phys_device(seg->device));
      if (e == hipSuccess && !col.h_dir.empty()) {
        e = hipMalloc((void**)&col.d_dir, col.h_dir.size() * sizeof(DevContainer));
        if (e == hipSuccess) e = hipMemcpy(col.d_dir, col.h_dir.data(), col.h_dir.size() * sizeof(DevContainer), hipMemcpyHostToDevice);
      }
      if (e != hipSuccess) return bail(fail(PG_ERR_DEVICE, "column %s: inverted index upload: %s", col.name.c_str(), hipGetErrorString(e)));
      col.inv_size = cd.inv_size;
      seg->device_bytes += cd.inv_size + col.h_dir.size() * sizeof(DevContainer);
    }
    if (cd.null_data && cd.null_size) {
      // NullValueVectorReaderImpl.getNullBitmap (NullValueVectorReaderImpl.java:44-46): the whole buffer is one RoaringBitmap.  It is
      // expanded once into a doc-order bitmap that IS_NULL leaves and the null-skipping aggregation lanes read like a posting.
      std::vector<DevContainer> dir;
      st = parse_roaring((const uint8_t*)cd.null_data, 0, cd.null_size, &dir);
      if (st != PG_OK) return bail(st);
      const long long words = (long long)std::max(seg->num_tiles, 1) * kMaxTileSteps;
      int64_t nulls = 0;
      std::vector<DevContainer> kept;
      for (const DevContainer& dc : dir) {
        if ((long long)dc.key * 1024 >= words) continue;   // containers beyond numDocs cannot hold a docId of this segment
        kept.push_back(dc);
        nulls += dc.cardinality;
      }
      if (nulls > 0) {
        uint8_t* d_bytes = nullptr;
        DevContainer* d_cont = nullptr;
        hipError_t e = hipMalloc((void**)&d_bytes, (size_t)cd.null_size + 16);
        if (e == hipSuccess) e = hipMemcpy(d_bytes, cd.null_data, (size_t)cd.null_size, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc((void**)&d_cont, kept.size() * sizeof(DevContainer));
        if (e == hipSuccess) e = hipMemcpy(d_cont, kept.data(), kept.size() * sizeof(DevContainer), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc((void**)&col.d_null_bitmap, (size_t)words * 8);
        if (e == hipSuccess) {
          roaring_expand_kernel<<<dim3((unsigned)((words + 1023) / 1024)), dim3(kBlockThreads), 0, 0>>>(d_bytes, d_cont, 0, (int)kept.size(), col.d_null_bitmap, words, 0);
          e = hipDeviceSynchronize();
        }
        if (d_bytes) (void)hipFree(d_bytes);
        if (d_cont) (void)hipFree(d_cont);
        if (e != hipSuccess) return bail(fail(PG_ERR_DEVICE, "column %s: null value vector upload: %s", col.name.c_str(), hipGetErrorString(e)));
        col.num_nulls = nulls;
        seg->device_bytes += (uint64_t)words * 8;
      }
    }
  }
  seg->num_user_cols = (int)seg->cols.size();
  seg->cols.reserve(seg->cols.size() * 3);      // hidden images are appended (at most two per column); the vector never reallocates after open
  // Raw INT / LONG columns as group keys: the value range (one pass over the resident column), and -- when it fits the int dictId
  // domain -- a placeholder for the column's KEY IMAGE, the fixed-bit stream of (value - min) that ensure_key_image builds the first
  // time the column is grouped by (pg_kernels.h, build_raw_key_image_kernel).  Nullable ones are built right away: their null-key image
  // below is made from it.
  {
    long long* d_mm = nullptr;
    for (int i = 0; i < seg->num_user_cols; ++i) {
      ColumnDev& col = seg->cols[(size_t)i];
      if (col.encoding != PG_FWD_RAW_FIXED_BYTE || seg->num_docs <= 0) continue;
      auto rank_placeholder = [&] {
        ColumnDev image;
        image.name = col.name + "$rankimage";
        image.stored_type = col.stored_type; image.encoding = PG_FWD_FIXED_BIT_DICT; image.vkind = kValI32;
        image.cardinality = 0; image.bits = 0; image.rank_image = true;
        image.key_image_of = i;
        col.keyimage_column = (int)seg->cols.size();
        seg->cols.push_back(std::move(image));
      };
      if (col.vkind != kValI32 && col.vkind != kValI64) { rank_placeholder(); continue; }      // FLOAT / DOUBLE: keyed by value through a rank image (pg_rank_image.h)
      long long mm[2] = {0x7FFFFFFFFFFFFFFFll, (long long)0x8000000000000000ull};
      hipError_t e = d_mm ? hipSuccess : hipMalloc((void**)&d_mm, 16);
      if (e == hipSuccess) e = hipMemcpy(d_mm, mm, 16, hipMemcpyHostToDevice);
      if (e == hipSuccess) {
        raw_min_max_kernel<<<dim3((unsigned)std::max(1, std::min(seg->num_docs / 1024 + 1, seg->num_cus * 8))), dim3(256), 0, 0>>>(col.d_fwd, col.vkind == kValI32 ? 4 : 8, seg->num_docs, d_mm);
        e = hipMemcpy(mm, d_mm, 16, hipMemcpyDeviceToHost);
      }
      if (e != hipSuccess) { if (d_mm) (void)hipFree(d_mm); return bail(fail(PG_ERR_DEVICE, "column %s: value range: %s", col.name.c_str(), hipGetErrorString(e))); }
      col.raw_min = mm[0]; col.raw_max = mm[1];
      if ((unsigned long long)mm[1] - (unsigned long long)mm[0] >= 0x7FFFFFFEull) { rank_placeholder(); continue; }      // max - min + 1 is not an int (with room for a null digit): a rank image instead
      ColumnDev image;
      image.name = col.name + "$keyimage";
      image.stored_type = col.stored_type; image.encoding = PG_FWD_FIXED_BIT_DICT; image.vkind = kValI32;
      image.cardinality = (int)(mm[1] - mm[0] + 1);
      image.bits = 1;
      while (image.bits < 31 && (1ll << image.bits) < (long long)image.cardinality) ++image.bits;      // PinotDataBitSet.getNumBitsPerValue(cardinality - 1)
      image.key_image_of = i; image.key_base = mm[0];
      col.keyimage_column = (int)seg->cols.size();
      seg->cols.push_back(std::move(image));
    }
    if (d_mm) (void)hipFree(d_mm);
    for (int i = 0; i < seg->num_user_cols; ++i) {
      if (seg->cols[(size_t)i].keyimage_column < 0 || !seg->cols[(size_t)i].d_null_bitmap) continue;
      if (seg->cols[(size_t)seg->cols[(size_t)i].keyimage_column].rank_image) continue;      // (no null-key image of a rank image: such a key under null handling stays with the CPU plan)
      const pg_status kst = ensure_key_image(seg, i, nullptr);
      if (kst != PG_OK) return bail(kst);
    }
  }
  // GROUP BY under enableNullHandling treats NULL as a key of its own (DefaultGroupByExecutor.java:106-121: the no-dictionary key
  // generators).  A nullable dictionary column therefore gets a second forward index whose dictId is `cardinality` wherever the doc is
  // null: the group-by kernels then need no notion of null (execute_null_handling points the key at this image).  A nullable raw
  // INT / LONG column gets the same image, made from its key image.
  for (int i = 0; i < seg->num_user_cols; ++i) {
    if (!seg->cols[(size_t)i].d_null_bitmap) continue;
    const int src = seg->cols[(size_t)i].encoding == PG_FWD_FIXED_BIT_DICT ? i : seg->cols[(size_t)i].keyimage_column;
    if (src < 0 || seg->cols[(size_t)src].rank_image) continue;
    int bits_out = 1;
    while (bits_out < 31 && (1ll << bits_out) <= (long long)seg->cols[(size_t)src].cardinality) ++bits_out;      // PinotDataBitSet.getNumBitsPerValue(cardinality)
    ColumnDev image;
    const ColumnDev& col = seg->cols[(size_t)src];
    image.key_image_of = col.key_image_of; image.key_base = col.key_base;      // (null-key image of a key image: still min + digit, digit == cardinality - 1 is NULL)
    image.name = seg->cols[(size_t)i].name + "$nullkey";
    image.stored_type = col.stored_type; image.encoding = col.encoding; image.vkind = col.vkind; image.value_base = col.value_base;
    image.bits = bits_out;
    image.cardinality = col.cardinality + 1;
    image.h_dict = col.h_dict; image.h_dict.push_back(0);
    image.h_dict_f64 = col.h_dict_f64; image.h_dict_f64.push_back(std::numeric_limits<double>::quiet_NaN());
    image.h_dict_i64 = col.h_dict_i64; if (!image.h_dict_i64.empty()) image.h_dict_i64.push_back(0);
    image.d_dict = col.d_dict; image.d_dict64 = col.d_dict64; image.borrows_dictionary = true;      // never gathered: the image is only ever a group key
    image.fwd_alloc_bytes = (size_t)std::max(seg->num_tiles, 1) * 256 * (size_t)bits_out + 64;
    hipError_t e = hipMalloc((void**)&image.d_fwd_alloc, image.fwd_alloc_bytes);
    if (e == hipSuccess) e = hipMemset(image.d_fwd_alloc, 0, image.fwd_alloc_bytes);
    if (e == hipSuccess) {
      build_nullkey_fwd_kernel<<<dim3((unsigned)std::max(1, std::min(seg->num_tiles / 4 + 1, seg->num_cus * 8))), dim3(256), 0, 0>>>(col.d_fwd, col.bits, seg->cols[(size_t)i].d_null_bitmap, image.d_fwd_alloc,
                                                                                                                                     bits_out, (uint32_t)col.cardinality, seg->num_tiles);
      e = hipDeviceSynchronize();
    }
    if (e != hipSuccess) { if (image.d_fwd_alloc) (void)hipFree(image.d_fwd_alloc); return bail(fail(PG_ERR_DEVICE, "column %s: null-key image: %s", col.name.c_str(), hipGetErrorString(e))); }
    image.d_fwd = image.d_fwd_alloc;
    seg->device_bytes += image.fwd_alloc_bytes;
    seg->cols[(size_t)i].nullkey_column = (int)seg->cols.size();
    seg->cols.push_back(std::move(image));
  }
  // Everything enqueued above (null-stream memsets of the padding, the posting expansion) has run before the first query can: the
  // queries' streams are non-blocking, they do not wait for the null stream by themselves.
  {
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return bail(fail(PG_ERR_DEVICE, "opening segment %s: %s", seg->name.c_str(), hipGetErrorString(e)));
  }
  *out_segment = seg;
  return PG_OK;
}

pg_status pg_segment_close(pg_segment* segment) {
  if (!segment) return fail(PG_ERR_INVALID_ARGUMENT, "null segment");
  (void)hipSetDevice(phys_device(segment->device));
  free_segment(segment);
  return PG_OK;
}

pg_status pg_segment_num_docs(const pg_segment* segment, int32_t* out_num_docs) {
  if (!segment || !out_num_docs) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  *out_num_docs = segment->num_docs;
  return PG_OK;
}

pg_status pg_segment_device_bytes(const pg_segment* segment, uint64_t* out_bytes) {
  if (!segment || !out_bytes) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  *out_bytes = segment->device_bytes.load(std::memory_order_relaxed);
  return PG_OK;
}

pg_status pg_group_key_info(const pg_segment* segment, int32_t column, int64_t* out_base, int32_t* out_is_offset, int32_t* out_null_entry) {
  if (!segment || !out_base || !out_is_offset || !out_null_entry) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  if (column < 0 || column >= segment->num_user_cols) return fail(PG_ERR_INVALID_ARGUMENT, "column %d out of range", column);
  const ColumnDev& col = segment->cols[(size_t)column];
  *out_base = 0; *out_is_offset = 0; *out_null_entry = col.cardinality;
  if (col.encoding == PG_FWD_FIXED_BIT_DICT) return PG_OK;
  if (col.keyimage_column < 0) return fail(PG_ERR_UNSUPPORTED, "group-by on raw column %s: no key image", col.name.c_str());
  const ColumnDev& image = segment->cols[(size_t)col.keyimage_column];
  if (image.rank_image) {
    // keyed by value through the column's own dictionary: an entry is a RANK, the values come from pg_group_key_values
    // (the NULL entry is the cardinality: known once the dictionary exists -- built here when no query has grouped by the column yet)
    const pg_status rst = ensure_key_image(const_cast<pg_segment*>(segment), column, nullptr);
    if (rst != PG_OK) return rst;
    *out_base = 0; *out_is_offset = 2; *out_null_entry = image.cardinality;
    return PG_OK;
  }
  *out_base = col.raw_min; *out_is_offset = 1; *out_null_entry = image.cardinality;
  return PG_OK;
}

pg_status pg_group_key_values(pg_segment* segment, int32_t column, int64_t* out_value_bits, int32_t capacity, int32_t* out_count) {
  if (!segment || !out_count) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  if (column < 0 || column >= segment->num_user_cols) return fail(PG_ERR_INVALID_ARGUMENT, "column %d out of range", column);
  ColumnDev& col = segment->cols[(size_t)column];
  if (col.keyimage_column < 0 || !segment->cols[(size_t)col.keyimage_column].rank_image)
    return fail(PG_ERR_INVALID_ARGUMENT, "column %s is not keyed through a rank image (pg_group_key_info: is_offset != 2)", col.name.c_str());
  const pg_status st = ensure_key_image(segment, column, nullptr);
  if (st != PG_OK) return st;
  const ColumnDev& image = segment->cols[(size_t)col.keyimage_column];
  *out_count = image.cardinality;
  if (!out_value_bits) return PG_OK;                                   // (sizing call)
  if (capacity < image.cardinality) return fail(PG_ERR_INVALID_ARGUMENT, "room for %d values, the column has %d distinct ones", capacity, image.cardinality);
  const bool floating = col.vkind == kValF32 || col.vkind == kValF64;
  for (int d = 0; d < image.cardinality; ++d) out_value_bits[d] = rank_image_value_bits(image.h_rank_keys[(size_t)d], floating);
  return PG_OK;
}

// What pg_result.internal points at: the dictId sets of the result's PG_AGG_DISTINCTCOUNT aggregations (pg_result_distinct_dict_ids).
struct DistinctSet {
  int aggregation = 0;                  // index into pg_query.aggregations
  int num_words = 0;                    // ceil(cardinality / 32)
  int rows = 1;
  std::vector<uint32_t> words;          // [rows * num_words]: one row (aggregation only), or one per row of group_aggregations
};
// The value list behind a PG_AGG_PERCENTILE aggregation, sparse and in dictionary order (pg_result_percentile_counts): row r holds the pairs
// [offsets[r], offsets[r + 1]) of (dict_ids, counts) -- ascending dictIds with a non-zero count.
struct CountList {
  int aggregation = 0;
  int rows = 1;                         // one (aggregation only), or one per row of group_aggregations
  std::vector<size_t> offsets;          // [rows + 1]
  std::vector<int32_t> dict_ids;
  std::vector<uint32_t> counts;
};
// `distinct` also carries the counts pass's dense counter rows (num_words = the cardinality) from harvest_sets to execute_percentile, which
// compacts them into `counts`: the dense matrix does not outlive pg_execute.
// The values behind a PG_AGG_PERCENTILE / PG_AGG_DISTINCTCOUNT aggregation on a raw column, as sorted runs (pg_result_value_counts): row r holds
// the runs [offsets[r], offsets[r + 1]) of (value_bits, counts).  From harvest_collect to execute_percentile / execute_distinct under GROUP BY the
// runs of ALL raw group ids travel in one row with run_rows beside them (ascending raw group id, then ascending value): finish_value_lists cuts
// them into the rows of the groups that exist.
struct ValueList {
  int aggregation = 0;
  int rows = 1;
  std::vector<size_t> offsets;          // [rows + 1]
  std::vector<int64_t> value_bits;      // the long value (INT / LONG), the IEEE-754 bits of the double (FLOAT widened / DOUBLE)
  std::vector<uint32_t> counts;
  std::vector<uint32_t> run_rows;       // in transit only: the raw group id of every run
  bool grouped_in_transit = false;
};
// The registers behind a PG_AGG_DISTINCTCOUNTHLL aggregation (pg_result_hll_registers): one rank per byte, 2^log2m bytes per row.
struct HllSet {
  int aggregation = 0;
  int log2m = 0;
  int rows = 1;                         // one (aggregation only), or one per row of group_aggregations (in transit from the pass: one per raw group id)
  std::vector<uint8_t> registers;       // [rows << log2m]
};
// The VarianceTuple behind a PG_AGG_VARIANCE aggregation (pg_result_moments).  In transit from the pass: m2 holds {S1, S2} per raw group id.
struct MomentsSet {
  int aggregation = 0;
  int rows = 1;                         // one (aggregation only), or one per row of group_aggregations
  std::vector<double> m2;               // [rows] (in transit: [rows x 2])
};
struct ResultInternal { std::vector<DistinctSet> distinct; std::vector<CountList> counts; std::vector<ValueList> values; std::vector<HllSet> hll; std::vector<MomentsSet> moments; };

void pg_result_free(pg_result* r) {
  if (!r) return;
  delete static_cast<ResultInternal*>(r->internal);
  free(r->aggregations);
  free(r->group_ids);
  free(r->group_ids64);
  free(r->group_key_dict_ids);
  free(r->group_aggregations);
  memset(r, 0, sizeof(*r));
}

constexpr int32_t kQueryHashHolder = 1 << 30;      // internal pg_query.flags bit (execute_null_handling -> execute_impl)
// internal pg_query.flags bit (execute_null_handling -> execute_impl): COUNT(column) keeps its input expression under enableNullHandling whether
// or not the column has null docs (CountAggregationFunction.getInputExpressions :69-71), so the column is projected and counts in
// numEntriesScannedPostFilter; without the option COUNT(column) is COUNT(*) and reads nothing
constexpr int32_t kQueryCountReadsColumn = 1 << 29;
// internal pg_query.flags bit (execute_distinct -> execute_impl): the bitset pass of a PG_AGG_DISTINCTCOUNT query.  Its aggregations are COUNT(*)
// and DISTINCTCOUNT only; group_by_columns are the key columns of group_distinct_kernel (the pass itself is an aggregation-only launch:
// which groups exist, and every other function, is the ordinary query's business -- check_distinct_plan / execute_distinct).
constexpr int32_t kQueryDistinctPass = 1 << 28;
// internal pg_query.flags bit (execute_percentile -> execute_impl): the counts pass of a PG_AGG_PERCENTILE query -- the bitset pass's shape with
// COUNT(*) and PERCENTILE aggregations, launched as scan_counts_kernel / group_counts_kernel (pg_scan_counts.h).  Never together with kQueryDistinctPass.
constexpr int32_t kQueryCountsPass = 1 << 27;
// internal pg_query.flags bit, set beside one of the two above: the pass's columns are RAW columns -- their values are collected into lists, sorted
// and run-length encoded (scan_collect_kernel / group_collect_kernel, pg_scan_collect.h) instead of counted per dictId.
constexpr int32_t kQueryCollectPass = 1 << 26;
// internal pg_query.flags bit, set beside kQueryDistinctPass: the pass's aggregations are DISTINCTCOUNTHLLs on RAW columns -- one launch of scan_hll_kernel /
// group_hll_kernel (pg_scan_hll.h) builds their registers.  (HLLs on dictionary columns ride the bitset pass itself: hll_fold_kernel behind its kernel.)
constexpr int32_t kQueryHllPass = 1 << 25;
// internal pg_query.flags bit, set beside kQueryDistinctPass: the pass's aggregations are PG_AGG_VARIANCEs on raw or dictionary columns -- one launch of
// scan_moments_kernel / group_moments_kernel (pg_scan_moments.h) accumulates their moments around the pivots execute_moments took from the ordinary query.
constexpr int32_t kQueryMomentsPass = 1 << 24;
constexpr int32_t kQuerySetPass = kQueryDistinctPass | kQueryCountsPass;
static inline bool is_moments_function(int32_t function) { return function == PG_AGG_VARIANCE; }
static inline bool is_hll_function(int32_t function) { return (function & 0xFF) == PG_AGG_DISTINCTCOUNTHLL; }
// the one function besides COUNT(*) a pass query carries, -1: not a pass
static inline int set_pass_function(int32_t flags) { return (flags & kQueryCountsPass) ? PG_AGG_PERCENTILE : ((flags & kQueryDistinctPass) ? PG_AGG_DISTINCTCOUNT : -1); }

// ---- plan-time eligibility (pg_query_check) ----
// Every reason pg_execute can answer PG_ERR_UNSUPPORTED for, decided from the query and the segment's metadata alone: no context, no
// allocation, no launch.  pg_execute runs it first, so both entry points reject the same queries; the same conditions further down the
// execution path are safety nets behind it.  Where the exact resource use depends on run-time state (which summed columns read a
// value plane decides how many column streams a query stages) the check takes the upper bound: it may decline a query whose streams
// would just have fitted, never the other way round.  InstancePlanMakerImplV2.makeSegmentPlanNode (:270-289) is where the caller asks.
// Group-by key spaces beyond an int: the reference's LongMapBasedHolder (the raw key fits a long) and ArrayMapBasedHolder (it does not)
// -- DictionaryBasedGroupKeyGenerator.java:162-176.  Here: a hashed table in HBM (GroupParams.hash_*), sized at plan time to at least
// twice the keys that can exist (min(numDocs, product)), so that it cannot fill up at run time.
// numGroupsLimit, with the reference's default (InstancePlanMakerImplV2.DEFAULT_NUM_GROUPS_LIMIT)
static inline int groups_limit(const pg_query* q) { return q->num_groups_limit > 0 ? q->num_groups_limit : 100000; }
struct HashPlan {
  int kind = 0;                    // 0: int raw keys (direct-indexed table); 1: long raw keys; 2: beyond a long (chained tables)
  int levels = 0;                  // first tables of a key beyond a long: table l takes over at column split[l]
  int split[kMaxHashLevels] = {};
  long long slots = 0, slots_lvl[kMaxHashLevels] = {};
  unsigned long long mult[kMaxGroupCols] = {};
  long long level_slots() const { long long t = 0; for (int l = 0; l < levels; ++l) t += slots_lvl[l]; return t; }
  int segment_begin(int l) const { return l == 0 ? 0 : split[l - 1]; }        // key l (l in [0, levels]) covers columns [segment_begin(l), segment_end(l, n))
  int segment_end(int l, int n) const { return l < levels ? split[l] : n; }
};
static pg_status plan_hash_holder(const pg_segment* seg, const std::vector<int>& cards, HashPlan* hp) {
  *hp = HashPlan();
  // the product of up to kMaxGroupCols 31-bit cardinalities does not fit 128 bits: saturate far above anything compared against
  const unsigned __int128 kSat = (unsigned __int128)1 << 100;
  auto sat_mul = [&](unsigned __int128 a, unsigned __int128 b) { return (a >= kSat || b >= kSat || a * b >= kSat) ? kSat : a * b; };
  unsigned __int128 prod = 1;
  for (int c : cards) prod = sat_mul(prod, (unsigned __int128)std::max(c, 1));
  if (prod <= (unsigned __int128)kMaxGroupSlots) return PG_OK;
  if ((long long)seg->num_docs > (1ll << 29))
    return fail(PG_ERR_UNSUPPORTED, "group-by with raw keys beyond an int on a segment of more than 2^29 docs (the hashed table would need more than 2^30 slots)");
  auto pow2_at_least = [](unsigned __int128 v) { long long p = 1 << 16; while ((unsigned __int128)p < v) p <<= 1; return p; };
  const int n = (int)cards.size();
  const unsigned __int128 kLongMax = (unsigned __int128)0x7FFFFFFFFFFFFFFFull;
  hp->kind = prod > kLongMax ? 2 : 1;
  hp->slots = pow2_at_least(2 * std::min<unsigned __int128>((unsigned __int128)seg->num_docs, prod));
  // Columns are taken in order while the key so far still fits a long; when the next column would push it beyond, the key so far goes
  // through a first table and its slot number (< 2^30) stands for it from there on (slot * card always fits: 2^30 * 2^31).
  unsigned __int128 bound = 1;             // exclusive upper bound of the running key
  unsigned __int128 seen = 1;              // distinct keys the columns so far can form
  for (int c = 0; c < n; ++c) {
    const unsigned __int128 card = (unsigned __int128)std::max(cards[(size_t)c], 1);
    if (bound * card > kLongMax) {
      if (hp->levels == kMaxHashLevels) return fail(PG_ERR_UNSUPPORTED, "group-by raw key needs more than %d chained tables", kMaxHashLevels);
      const long long s = pow2_at_least(2 * std::min<unsigned __int128>((unsigned __int128)seg->num_docs, seen));
      hp->split[hp->levels] = c; hp->slots_lvl[hp->levels] = s; hp->levels++;
      bound = (unsigned __int128)s;
    }
    hp->mult[c] = (unsigned long long)bound;
    bound *= card;
    seen = sat_mul(seen, card);
  }
  return PG_OK;
}

static pg_status check_query_plan(const pg_segment* seg, const pg_query* q, int extra_and_leaves) {
  const int num_cols_total = (int)seg->cols.size();
  if (q->num_filter_nodes < 0 || q->num_filter_nodes > kMaxNodes) return fail(PG_ERR_UNSUPPORTED, "filter tree has %d nodes (max %d)", q->num_filter_nodes, kMaxNodes);
  if (q->num_filter_nodes > 0 && (!q->filter || !q->predicates)) return fail(PG_ERR_INVALID_ARGUMENT, "filter nodes without predicates");
  std::vector<int> filter_cols;           // columns whose stream a scan leaf stages
  {
    int depth = 0;
    for (int n = 0; n < q->num_filter_nodes; ++n) {
      const pg_filter_node& fn = q->filter[n];
      if (fn.op == PG_FILTER_LEAF) {
        if (fn.predicate < 0 || fn.predicate >= q->num_predicates) return fail(PG_ERR_INVALID_ARGUMENT, "filter node %d: bad predicate index", n);
        depth++;
      } else if (fn.op == PG_FILTER_NOT) {
        if (depth < 1) return fail(PG_ERR_INVALID_ARGUMENT, "malformed filter tree (node %d)", n);
      } else if (fn.op == PG_FILTER_AND || fn.op == PG_FILTER_OR) {
        if (fn.num_children < 1 || depth < fn.num_children) return fail(PG_ERR_INVALID_ARGUMENT, "malformed filter tree (node %d)", n);
        depth -= fn.num_children - 1;
      } else return fail(PG_ERR_INVALID_ARGUMENT, "unknown filter op %d", fn.op);
    }
    if (q->num_filter_nodes > 0 && depth != 1) return fail(PG_ERR_INVALID_ARGUMENT, "malformed filter tree (%d roots)", depth);
    // the same re-ordering lower_filter applies: the root AND as a chain, its inverted-index children as one leaf
    std::vector<SeqNode> seq;
    std::vector<int> and_members;
    int lazy_node = -1, num_bitmap_prefix = 0;
    build_sequence(q, &seq, &lazy_node, &num_bitmap_prefix, &and_members);
    if ((int)seq.size() + 2 * extra_and_leaves > kMaxNodes) return fail(PG_ERR_UNSUPPORTED, "filter tree has %d nodes (max %d)", (int)seq.size() + 2 * extra_and_leaves, kMaxNodes);
    int leaves = extra_and_leaves, max_depth = extra_and_leaves > 0 ? 2 : 0;
    depth = 0;
    for (const SeqNode& sn : seq) {
      if (sn.op == PG_FILTER_LEAF) { leaves++; depth++; }
      else if (sn.op != PG_FILTER_NOT) depth -= sn.num_children - 1;
      max_depth = std::max(max_depth, depth);
      if (sn.op == PG_FILTER_LEAF && sn.src >= 0) {
        const pg_predicate& pr = q->predicates[q->filter[sn.src].predicate];
        if (pr.kind == PG_PRED_RAW_SET) {
          std::vector<uint64_t> keys;
          const pg_status rst = check_raw_set(seg, pr, &keys);
          if (rst != PG_OK) return rst;
        }
        if (pr.kind == PG_PRED_DOC_SET && !find_doc_set(seg, pr.lo))
          return fail(PG_ERR_INVALID_ARGUMENT, "doc set %lld is unknown to segment %s (never created, or released)", (long long)pr.lo, seg->name.c_str());
        const bool stages = pr.kind == PG_PRED_RAW_RANGE || ((pr.kind == PG_PRED_DICT_RANGE || pr.kind == PG_PRED_DICT_SET) && pr.eval != PG_EVAL_INVERTED);
        if (stages) {
          if (pr.column < 0 || pr.column >= num_cols_total) return fail(PG_ERR_INVALID_ARGUMENT, "predicate column %d out of range", pr.column);
          if (std::find(filter_cols.begin(), filter_cols.end(), pr.column) == filter_cols.end()) filter_cols.push_back(pr.column);
        }
      }
    }
    if (leaves > kMaxLeaves) return fail(PG_ERR_UNSUPPORTED, "more than %d filter leaves", kMaxLeaves);
    if (max_depth + (extra_and_leaves > 0 ? 1 : 0) > kStackDepth) return fail(PG_ERR_UNSUPPORTED, "filter tree deeper than %d", kStackDepth);
  }
  const int pass_function = set_pass_function(q->flags);
  const bool distinct_pass = pass_function >= 0;      // the bitset / counts pass (its keys were checked with the ordinary query: plan_distinct / plan_percentile)
  const int na = q->num_aggregations, ng = distinct_pass ? 0 : q->num_group_by;
  if (na < 0 || ng < 0 || (na > 0 && !q->aggregations) || (ng > 0 && !q->group_by_columns)) return fail(PG_ERR_INVALID_ARGUMENT, "bad aggregation / group-by lists");
  if (ng > kMaxGroupCols) return fail(PG_ERR_UNSUPPORTED, "more than %d group-by columns", kMaxGroupCols);
  std::vector<int> key_cols, agg_cols, key_cards;
  long long product = 1;
  for (int g = 0; g < ng; ++g) {
    int c = q->group_by_columns[g];
    if (c < 0 || c >= num_cols_total) return fail(PG_ERR_INVALID_ARGUMENT, "group-by column %d out of range", c);
    if (seg->cols[(size_t)c].encoding != PG_FWD_FIXED_BIT_DICT) {
      // a raw INT / LONG column is grouped by through its key image (cardinality and width are known since open; nothing is built here)
      if (seg->cols[(size_t)c].keyimage_column < 0)
        return fail(PG_ERR_UNSUPPORTED, "group-by on raw column %s: no key image", seg->cols[(size_t)c].name.c_str());
      if (seg->cols[(size_t)seg->cols[(size_t)c].keyimage_column].rank_image) {
        // a rank image's cardinality is what the plan is priced with: the column's dictionary is built here, the first time a query that
        // groups by it is checked (once per column and segment; the one thing pg_query_check ever launches)
        // A build that fails -- no HBM for its transient keys, a device error -- is a reason to keep the CPU plan, not to fail a query at PLAN
        // time: the JNI layer throws on every status but OK / UNSUPPORTED and GpuPlanMaker.makeSegmentPlanNode lets that through (advisor, round 5).
        const pg_status rst = ensure_key_image(const_cast<pg_segment*>(seg), c, nullptr);
        if (rst != PG_OK) {
          (void)hipGetLastError();
          return fail(PG_ERR_UNSUPPORTED, "group-by on raw column %s: its dictionary and rank image could not be built (status %d: %s) -- CPU plan", seg->cols[(size_t)c].name.c_str(), (int)rst,
                      pg_last_error());
        }
      }
      c = seg->cols[(size_t)c].keyimage_column;
    }
    const ColumnDev& col = seg->cols[(size_t)c];
    key_cards.push_back(col.cardinality);
    if (std::find(key_cols.begin(), key_cols.end(), c) == key_cols.end()) key_cols.push_back(c);
  }
  HashPlan hash_plan;
  if (ng > 0) { const pg_status hst = plan_hash_holder(seg, key_cards, &hash_plan); if (hst != PG_OK) return hst; }
  if (hash_plan.kind == 0) for (int card : key_cards) product *= std::max(card, 1);
  else {
    // Long / ArrayMap holders run in the lane-private group-by kernel only: 32-bit-domain aggregations, lane-private filter leaves
    product = hash_plan.slots;
    if (q->flags & kQueryHashHolder) return fail(PG_ERR_UNSUPPORTED, "group-by with raw keys beyond an int under null handling (plan-time fallback)");
    for (int n = 0; n < q->num_filter_nodes; ++n) {
      if (q->filter[n].op != PG_FILTER_LEAF) continue;
      const pg_predicate& pr = q->predicates[q->filter[n].predicate];
      if (pr.kind == PG_PRED_RAW_RANGE && pr.column >= 0 && pr.column < num_cols_total && seg->cols[(size_t)pr.column].stored_type != PG_TYPE_INT)
        return fail(PG_ERR_UNSUPPORTED, "group-by with raw keys beyond an int under a raw 8-byte range predicate (plan-time fallback)");
    }
  }
  std::vector<std::pair<int, int>> group_aggs;     // distinct (column, SUM | MIN | MAX)
  for (int a = 0; a < na; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    if (distinct_pass ? (ag.function != PG_AGG_COUNT && ag.function != pass_function && !(pass_function == PG_AGG_DISTINCTCOUNT && is_hll_function(ag.function)) && !((q->flags & kQueryMomentsPass) && is_moments_function(ag.function))) : (ag.function < PG_AGG_COUNT || ag.function > PG_AGG_AVG))
      return fail(PG_ERR_UNSUPPORTED, "aggregation function %d", ag.function);
    if (ag.function == PG_AGG_COUNT) continue;
    if (ag.column < 0 || ag.column >= num_cols_total) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation column %d out of range", ag.column);
    if (std::find(agg_cols.begin(), agg_cols.end(), ag.column) == agg_cols.end()) agg_cols.push_back(ag.column);
    if (ng > 0) {
      const ColumnDev& col = seg->cols[(size_t)ag.column];
      const int kind = (ag.function == PG_AGG_SUM || ag.function == PG_AGG_AVG) ? 0 : (ag.function == PG_AGG_MIN ? 1 : 2);
      if (std::find(group_aggs.begin(), group_aggs.end(), std::make_pair(ag.column, kind)) == group_aggs.end()) group_aggs.emplace_back(ag.column, kind);
      if (kind == 2 && dict_ends_in_nan(col)) return fail_group_max_over_nan_dictionary(col.name.c_str());
      if (col.encoding == PG_FWD_RAW_FIXED_BYTE && col.vkind != kValI32) {
        // group_typed_direct_kernel takes it, with the lane-private filter: a range leaf on a raw 8-byte column is not in that filter
        for (int n = 0; n < q->num_filter_nodes; ++n) {
          if (q->filter[n].op != PG_FILTER_LEAF) continue;
          const pg_predicate& pr = q->predicates[q->filter[n].predicate];
          if (pr.kind == PG_PRED_RAW_RANGE && pr.column >= 0 && pr.column < num_cols_total && seg->cols[(size_t)pr.column].stored_type != PG_TYPE_INT)
            return fail(PG_ERR_UNSUPPORTED, "group-by aggregation of a raw 8-byte column under a raw 8-byte range predicate (plan-time fallback)");
        }
      }
      // (an 8-byte input under a hashed holder -- RAW, or the SUM of a dictionary column with 8-byte values -- takes group_typed_direct_kernel<.., kHash>: round 6b)
      if (kind == 0 && col.vkind == kValI64 && !col.h_dict_i64.empty()) {
        const double max_abs = std::max(std::fabs((double)col.h_dict_i64.front()), std::fabs((double)col.h_dict_i64.back()));
        if ((double)seg->num_docs * max_abs >= 9.2e18) return fail(PG_ERR_UNSUPPORTED, "group-by SUM of LONG column %s could overflow int64", col.name.c_str());
      }
    }
  }
  if (ng == 0 && (int)agg_cols.size() > kMaxAggCols) return fail(PG_ERR_UNSUPPORTED, "more than %d aggregated columns", kMaxAggCols);
  if ((int)group_aggs.size() > kMaxGroupAggs) return fail(PG_ERR_UNSUPPORTED, "more than %d distinct group-by aggregations", kMaxGroupAggs);
  if (ng > 0 && ((unsigned long long)product * (1ull + group_aggs.size() + (hash_plan.kind ? 1 : 0)) + (unsigned long long)hash_plan.level_slots()) * 8ull > g_engine.group_table_bytes)
    return fail(PG_ERR_UNSUPPORTED, "group-by table of %lld slots x %zu words exceeds the %llu-byte budget (PINOT_GPU_GROUP_TABLE_BYTES)", product, 1 + group_aggs.size(),
                (unsigned long long)g_engine.group_table_bytes);
  // Column streams, as slot_for hands them out: (column, read through its value plane?).  A column summed through its plane is read
  // through the plane by everything that can be (its other aggregations, a dictId-range leaf on it); set leaves and group keys read
  // the dictIds.  Which summed columns have a plane is want_value_plane's decision; the histogram path, which reads the dictIds
  // instead, is not anticipated here (run-time tiers): at worst one stream too many is counted.
  std::vector<char> plane((size_t)std::max(num_cols_total, 1), 0);
  for (int a = 0; a < na; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    if ((ag.function == PG_AGG_SUM || ag.function == PG_AGG_AVG) && (want_value_plane(seg->cols[(size_t)ag.column]) || want_wide_plane(seg, q, ag.column))) plane[(size_t)ag.column] = 1;
  }
  std::vector<int> streams;               // column * 2 + plane
  auto use = [&](int column, bool through_plane) {
    const int key = column * 2 + (through_plane ? 1 : 0);
    if (std::find(streams.begin(), streams.end(), key) == streams.end()) streams.push_back(key);
  };
  for (int n = 0; n < q->num_filter_nodes; ++n) {
    if (q->filter[n].op != PG_FILTER_LEAF) continue;
    const pg_predicate& pr = q->predicates[q->filter[n].predicate];
    if (pr.column < 0 || pr.column >= num_cols_total) continue;
    if (pr.kind == PG_PRED_RAW_RANGE) use(pr.column, false);
    else if (pr.kind == PG_PRED_DICT_RANGE && pr.eval != PG_EVAL_INVERTED) use(pr.column, plane[(size_t)pr.column] != 0);
    else if (pr.kind == PG_PRED_DICT_SET && pr.eval != PG_EVAL_INVERTED) use(pr.column, false);
  }
  for (int c : key_cols) use(c, false);
  if (distinct_pass) for (int g = 0; g < q->num_group_by; ++g) {
    const int c = q->group_by_columns[g];
    if (c >= 0 && c < num_cols_total) use(seg->cols[(size_t)c].encoding == PG_FWD_FIXED_BIT_DICT ? c : std::max(seg->cols[(size_t)c].keyimage_column, 0), false);
  }
  for (int c : agg_cols) use(c, plane[(size_t)c] != 0);
  const int bound = (int)streams.size();
  if (bound > kMaxCols) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
  return PG_OK;
}

// ExecutionStatistics.numEntriesScannedInFilter from the plan pg_filter_stats.h chose; `counted`: the kernel that ran carried the
// kNodeCountEntries counter (its value has been copied to ctx->h_filter_entries and the stream is idle).
static void finish_filter_stats(fstats::Plan stats_plan, int stats_scan_leaves, const pg_segment* seg, int64_t counted_entries, bool counted, pg_result* out) {
  const int64_t upper_bound = (int64_t)stats_scan_leaves * seg->num_docs;      // every scan leaf looking at every doc
  switch (stats_plan) {
    case fstats::Plan::kZero: out->stats.num_entries_scanned_in_filter = 0; out->filter_entries_exact = 1; break;
    case fstats::Plan::kPerLeaf: out->stats.num_entries_scanned_in_filter = upper_bound; out->filter_entries_exact = 1; break;
    case fstats::Plan::kLeap2:
      // one entry per doc for whichever leaf is scanning there, plus the device's count of the docs where the other leaf was asked
      if (counted) { out->stats.num_entries_scanned_in_filter = (int64_t)seg->num_docs + counted_entries; out->filter_entries_exact = 1; break; }
      out->stats.num_entries_scanned_in_filter = upper_bound; out->filter_entries_exact = 0; break;
    case fstats::Plan::kChain:
      if (counted) { out->stats.num_entries_scanned_in_filter = counted_entries; out->filter_entries_exact = 1; break; }
      [[fallthrough]];                                                            // an LDS-staged kernel ran: replayed by pg_execute
    default: out->stats.num_entries_scanned_in_filter = upper_bound; out->filter_entries_exact = 0; break;
  }
}

static void finish_filter_stats(const Lowered& lw, const pg_segment* seg, int64_t counted_entries, bool counted, pg_result* out) {
  if (lw.stats_closed_entries >= 0) { out->stats.num_entries_scanned_in_filter = lw.stats_closed_entries; out->filter_entries_exact = 1; return; }
  finish_filter_stats(lw.stats_plan, lw.stats_scan_leaves, seg, counted_entries, counted, out);
}

// pg_execute_batch: a query whose whole device work is ONE launch of scan_private_kernel -- nothing ahead of it on the stream, no index
// phase, no entry counter, no histogram -- is not launched by execute_impl but handed back as its kernel parameters plus the
// conversion of the folded record into a pg_result; the batch puts many of them into one launch (scan_private_batch_kernel).
static const pg_status kDeferred = static_cast<pg_status>(100);      // (internal: never leaves the library)
static const pg_status kRunAlone = static_cast<pg_status>(101);      // (internal: a batch item whose shared launch could not answer it -- pg_execute_batch runs it by itself)
static const pg_status kHistRetry = static_cast<pg_status>(102);     // (internal: the histogram's counters could not answer -- execute_impl answers the query again)
// Kinds of shared launch (ScanParams.lean_kind): pg_execute_batch groups a batch's deferred items by device and kind, one launch each.
// Private: scan_private_batch_kernel (the general lane-private body); Simple / Raw / SimpleSet: scan_lean_batch_kernel<1 | 2 | 13> (the
// scan_simple / scan_raw shape, 13 with its one set leaf in LDS); Hist*: scan_hist_batch_kernel<8 | 16 | 32> (plain counters); GroupLds:
// group_lds_batch_kernel; Narrow*: scan_narrow_batch_kernel<general | single leaf>; Typed*: scan_typed_batch_kernel<1 | 2 | kMaxAggCols>
// (raw and 8-byte aggregated columns); IndexAnd: index_and_batch_kernel (the item's whole device work is index_and_kernel).
enum class BatchKind : int32_t { Private = 0, Simple = 1, Raw = 2, Hist8 = 3, Hist16 = 4, Hist32 = 5, GroupLds = 6, Narrow = 7, NarrowSingle = 8,
                                 Typed1 = 9, Typed2 = 10, TypedMax = 11, IndexAnd = 12, SimpleSet = 13 };
// What enqueue_deferred needs of a scan kind: workgroup waves, tiles a wave takes per iteration (the narrow kernels walk four / eight), counter
// bits, typed slots, and the waves per CU its kernel holds (0: Private, sized by PINOT_GPU_BATCH_BLOCKS_PER_CU).  GroupLds / IndexAnd: none.
struct BatchKindInfo { int block_waves = kBlockThreads / 64, tiles_per_wave = 1, hist_bits = 0, typed_slots = 0, wave_cap = 0; };
static BatchKindInfo batch_kind_info(BatchKind kind) {
  BatchKindInfo i;
  switch (kind) {
    case BatchKind::Hist8: case BatchKind::Hist16: case BatchKind::Hist32:
      i.block_waves = kHistBlockThreads / 64; i.hist_bits = kind == BatchKind::Hist8 ? 8 : (kind == BatchKind::Hist16 ? 16 : 32); i.wave_cap = waves_scan_hist_batch(i.hist_bits); break;
    case BatchKind::Narrow: case BatchKind::NarrowSingle:
      i.tiles_per_wave = kind == BatchKind::Narrow ? kNarrowTiles : kNarrowSingleTiles; i.wave_cap = waves_scan_narrow_batch(kind == BatchKind::NarrowSingle); break;
    case BatchKind::Typed1: case BatchKind::Typed2: case BatchKind::TypedMax:
      i.typed_slots = kind == BatchKind::Typed1 ? 1 : (kind == BatchKind::Typed2 ? 2 : kMaxAggCols); i.wave_cap = waves_scan_typed_batch(i.typed_slots); break;
    case BatchKind::Simple: case BatchKind::Raw: case BatchKind::SimpleSet: i.wave_cap = waves_scan_lean_batch((int)kind); break;
    default: break;
  }
  return i;
}
static void launch_batch_kind(BatchKind kind, const BatchKindInfo& i, bool one_slot, int blocks, size_t lds, hipStream_t stream, const ScanParams* items, const uint32_t* first, int n) {
  if (i.hist_bits) launch_scan_hist_batch(i.hist_bits, blocks, lds, stream, items, first, n);
  else if (i.tiles_per_wave > 1) launch_scan_narrow_batch(kind == BatchKind::NarrowSingle, blocks, stream, items, first, n);
  else if (i.typed_slots) launch_scan_typed_batch(i.typed_slots, blocks, stream, items, first, n);
  else if (kind != BatchKind::Private) launch_scan_lean_batch((int)kind, blocks, stream, items, first, n);
  else launch_scan_private_batch(one_slot, blocks, stream, items, first, n);
}
// A query lowered for the shared launch of pg_execute_batch: the kernel's parameter block (the launch fills in where this item's records
// go), the workgroups it would get on its own, and the conversion of its folded record into the reference's holder types.  Immutable
// once built: the segment's plan_cache hands the same item to later batches.
struct OwnedQuery {                               // a deep copy of a pg_query (the caller's arrays are only valid during its call)
  pg_query q;
  std::vector<pg_filter_node> filter;
  std::vector<pg_predicate> predicates;
  std::vector<std::vector<uint32_t>> set_words;
  std::vector<pg_aggregation> aggregations;
  std::vector<int32_t> group_by;
};
struct LoweredItem {
  ScanParams sp;
  int blocks = 0;
  bool one_slot = true;
  std::function<void(const BlockPartial&, pg_result*)> convert;
  std::vector<int> plane_columns;                 // value planes sp reads: held (PlaneHold) by every batch that launches this item
  std::vector<std::shared_ptr<DocSet>> doc_sets;  // doc sets sp reads: alive as long as the item (pg_doc_set_release drops the item from the plan cache)
  std::vector<Lowered::SetLeaf> sets;             // dictId-set leaves of sp: nodes whose set_words == ctx_words read the batch's copy of host_words (which the item's query owns)
  // lean_kind 6 (group_lds_batch_kernel): the item is a GroupParams; its table slice is count[G] | acc[NA][G], zero-identity keys
  std::shared_ptr<GroupParams> gp;
  int group_threads = 0;
  size_t group_lds = 0, group_table_words = 0;
  std::function<void(const unsigned long long*, pg_result*)> convert_group;      // the item's slice (on the host) -> the result
  // lean_kind 12 (index_and_batch_kernel): the item is an IndexAndParams whose kernel publishes the query's record (no ctx-owned memory in it)
  std::shared_ptr<IndexAndParams> and_params;
  uint32_t and_windows = 0;
  size_t hist_lds = 0;                            // lean_kind 3..5: the item's histogram (the launch's dynamic LDS is the largest item's)
  int hist_cw = 0, hist_col = -1;                 //   counter width; the summed column (a wrapped counter moves it to the guarded tier)
  // the cache's side (empty key: not cacheable)
  std::string key;                                // query_key of the query
  uint64_t engine_epoch = 0, plane_epoch = 0;
  std::shared_ptr<const OwnedQuery> query;        // `convert` reads the query through this copy
};
struct Deferred {
  std::shared_ptr<const LoweredItem> item;
  std::unique_ptr<PlaneHold> planes;           // value planes the kernel reads stay held until the batch has run
  bool cacheable = false;                      // out of execute_impl: nothing about this lowering was provisional
  bool single = false;                         // in: pg_execute's own call -- only a group-by of the LDS-table form is deferred (at any size), scans run as they always did
};

// The query's content as bytes: two queries with equal keys lower to the same item on the same segment.
static bool query_key(const pg_query* q, std::string* key) {
  key->clear();
  if (q->num_filter_nodes < 0 || q->num_predicates < 0 || q->num_aggregations < 0 || q->num_group_by < 0) return false;
  if ((q->num_filter_nodes > 0 && !q->filter) || (q->num_predicates > 0 && !q->predicates) || (q->num_aggregations > 0 && !q->aggregations) ||
      (q->num_group_by > 0 && !q->group_by_columns)) return false;
  const int32_t head[6] = {q->num_filter_nodes, q->num_predicates, q->num_aggregations, q->num_group_by, q->num_groups_limit, q->flags};
  key->append(reinterpret_cast<const char*>(head), sizeof(head));
  key->append(reinterpret_cast<const char*>(q->filter), sizeof(pg_filter_node) * (size_t)q->num_filter_nodes);
  for (int i = 0; i < q->num_predicates; ++i) {
    const pg_predicate& pr = q->predicates[i];
    if (pr.num_set_words < 0 || (pr.num_set_words > 0 && !pr.set_words)) { key->clear(); return false; }      // (an empty key = not cacheable)
    const int64_t fields[8] = {pr.kind, pr.column, pr.eval, pr.exclusive, pr.lo, pr.hi, pr.num_set_words, pr.reserved};
    key->append(reinterpret_cast<const char*>(fields), sizeof(fields));
    key->append(reinterpret_cast<const char*>(pr.set_words), sizeof(uint32_t) * (size_t)pr.num_set_words);
  }
  key->append(reinterpret_cast<const char*>(q->aggregations), sizeof(pg_aggregation) * (size_t)q->num_aggregations);
  key->append(reinterpret_cast<const char*>(q->group_by_columns), sizeof(int32_t) * (size_t)q->num_group_by);
  return true;
}

static std::shared_ptr<const OwnedQuery> own_query(const pg_query* q) {
  auto o = std::make_shared<OwnedQuery>();
  o->q = *q;
  if (q->num_filter_nodes > 0) o->filter.assign(q->filter, q->filter + q->num_filter_nodes);
  if (q->num_predicates > 0) o->predicates.assign(q->predicates, q->predicates + q->num_predicates);
  o->set_words.resize(o->predicates.size());
  for (size_t i = 0; i < o->predicates.size(); ++i) {
    pg_predicate& pr = o->predicates[i];
    if (pr.num_set_words > 0) { o->set_words[i].assign(pr.set_words, pr.set_words + pr.num_set_words); pr.set_words = o->set_words[i].data(); }
    else pr.set_words = nullptr;
  }
  if (q->num_aggregations > 0) o->aggregations.assign(q->aggregations, q->aggregations + q->num_aggregations);
  o->q.filter = o->filter.empty() ? nullptr : o->filter.data();
  o->q.predicates = o->predicates.empty() ? nullptr : o->predicates.data();
  o->q.aggregations = o->aggregations.empty() ? nullptr : o->aggregations.data();
  if (q->num_group_by > 0) o->group_by.assign(q->group_by_columns, q->group_by_columns + q->num_group_by);
  o->q.group_by_columns = o->group_by.empty() ? nullptr : o->group_by.data();
  return o;
}

static pg_status prepare_fsm_side(pg_segment* seg, ExecCtx* ctx, const pg::fstats::Fsm& fsm, FsmSide* side);
static pg_status device_fsm_filter_stats(pg_segment* seg, ExecCtx* ctx, const pg_query* q, const FsmSide& side, pg_result* out);
// PINOT_GPU_EXEC_TRACE=1: the host phases of every pg_execute on stderr -- eligibility check | context + lowering | launches enqueued | wait |
// result conversion (what a query's host clock is made of beside its kernels; execute_impl marks the boundaries it passes)
struct ExecTrace {
  std::chrono::steady_clock::time_point t[6];
  bool seen[6];
};
static thread_local ExecTrace t_exec_trace;
static bool exec_trace_on() { static const bool on = getenv("PINOT_GPU_EXEC_TRACE") != nullptr; return on; }
static inline void exec_mark(int i) {
  if (!exec_trace_on()) return;
  t_exec_trace.t[i] = std::chrono::steady_clock::now();
  t_exec_trace.seen[i] = true;
}

static pg_status execute_impl(pg_segment* seg, const pg_query* q, pg_result* out, unsigned long long* d_out_bitmap_request,
                              uint64_t* host_bitmap, int64_t host_bitmap_words, int64_t* out_cardinality, bool allow_metadata_plan = true,
                              Deferred* defer = nullptr, FsmSide* side = nullptr);

// ---- the aggregation-only path's kernel: one value per kernel the path launches.  choose_scan_kernel tries them in order of
// preference; the grid, the PG_KERNEL_* id, the kind of shared launch, the fold's flags and the launcher all follow from the choice.
enum class ScanKernel { Hist, Narrow, NarrowSingle, Sparse, Simple, SimpleSet, SimpleValid, Raw, RawSet, PrivateFsm, Private, PrivateTyped, Distinct, GroupDistinct, Counts, GroupCounts, Collect, GroupCollect, Hll, GroupHll, Moments, GroupMoments, Agg };
// per ScanKernel: its PG_KERNEL_* id, and whether it evaluates the filter with eval_filter_private over every tile (it can then leave the
// leaves' bitmaps for the transducer pass; PrivateFsm walks the transducer itself)
static const struct { int id; bool writes_leaves; } kScanKernels[] = {
  {PG_KERNEL_SCAN_HIST, true}, {PG_KERNEL_SCAN_NARROW, true}, {PG_KERNEL_SCAN_NARROW, false}, {PG_KERNEL_SCAN_SPARSE, false}, {PG_KERNEL_SCAN_SIMPLE, false},
  {PG_KERNEL_SCAN_SIMPLE, false}, {PG_KERNEL_SCAN_SIMPLE_VALID, false}, {PG_KERNEL_SCAN_RAW, false}, {PG_KERNEL_SCAN_RAW_SET, false}, {PG_KERNEL_SCAN_PRIVATE, false}, {PG_KERNEL_SCAN_PRIVATE, true},
  {PG_KERNEL_SCAN_PRIVATE_TYPED, true}, {PG_KERNEL_SCAN_DISTINCT, true}, {PG_KERNEL_GROUP_DISTINCT, true}, {PG_KERNEL_SCAN_COUNTS, true}, {PG_KERNEL_GROUP_COUNTS, true},
  {PG_KERNEL_SCAN_COLLECT, true}, {PG_KERNEL_GROUP_COLLECT, true}, {PG_KERNEL_SCAN_HLL, true}, {PG_KERNEL_GROUP_HLL, true}, {PG_KERNEL_SCAN_MOMENTS, true}, {PG_KERNEL_GROUP_MOMENTS, true}, {PG_KERNEL_SCAN_AGG, false}};
static_assert(sizeof(kScanKernels) / sizeof(kScanKernels[0]) == (size_t)ScanKernel::Agg + 1, "one row per ScanKernel");
// general: the kernel of the query's family -- Private or PrivateTyped, or Agg when neither lane-private kernel takes the query.  A
// specialised kernel that won keeps it: the index handling, the leap-frog count and the batch's fallbacks go by the family.
struct ScanChoice {
  ScanKernel kernel = ScanKernel::Agg, general = ScanKernel::Agg;
  int hist_slot = -1, hist_cw = 0;         // Hist: the aggregation slot the histogram counts, its counter bits ...
  bool hist_guarded = false;               // ... and whether they are the guarded tier's
  bool pipe = false;                       // Simple: scan_simple_pipe_kernel, the form with both columns' loads pipelined across tiles (same id, same batch kind)
  bool dma = false, dma_nt = false;        // Simple: scan_simple_dma_kernel, the two columns through a wave-private LDS ring (same id, same batch kind); goes before `pipe`
  bool dma_pair = false;                   // ... in its form with both widths compile-time constants (scan_simple_dma_pair_kernel)
  int dma_blocks_per_cu = 0;               // ... its workgroups per CU
};
// scan_simple_pipe_kernel always loads the aggregated column: it wins where scan_simple_kernel's lane skip and sparse walk have nothing to
// skip.  The leaf's selectivity is estimated as span / cardinality of its column (1 - that for an exclusive leaf); at or above this many
// per cent the pipelined form is taken (DESIGN.md 4.1g has the table the figure comes from).
constexpr int kPipeMinSelectivityPct = 5;
// scan_simple_dma_kernel (pg_scan_simple_dma.h) takes the pipelined kernel's queries -- same conditions, every width pair -- when a ring is
// worth filling and the shape is one that was measured: at least kDmaMinTilesPerWave tiles for every resident wave (2.4 lose to the pipelined
// kernel, 12 win), slots of at least kDmaMinSlotBytes (the headline's: what a wave keeps in flight is one slot, and narrower pairs were not
// measured) and room for kDmaBlocksPerCu workgroups of four waves per CU (one workgroup per CU is slower than the pipelined kernel: the
// decode of four waves does not cover the CU's stream).  Non-temporal loads when the two columns together exceed the Infinity Cache (a smaller
// segment queried again is served from it).  DESIGN.md 4.1g has the tables the figures come from.
// kDmaMinSlotBytes, kDmaBlocksPerCu and the LDS budget are pg_dma_pairs.h's: the pairs that pass them are the pairs scan_simple_dma_pair_kernel,
// the form with a straight-line tile, is instantiated for (dma_pair_admitted); every other pair the switch at 2 sends here keeps the generic form.
constexpr int kDmaMinTilesPerWave = 8;
static_assert(kDmaLdsBudget == kLdsBudget, "pg_dma_pairs.h prices the rings against this budget");
constexpr long long kInfinityCacheBytes = 256ll << 20;
static void plan_scan_simple_dma(const pg_segment* seg, int filter_bits, int value_bits, bool dense, ScanChoice* k) {
  const int bpc = std::min(blocks_scan_simple_dma(filter_bits, value_bits, kLdsBudget), g_engine.dma_blocks_per_cu > 0 ? g_engine.dma_blocks_per_cu : kDmaBlocksPerCu);
  if (bpc < 1) return;      // (does not happen: one workgroup's rings of the widest pair are half the budget)
  k->dma_blocks_per_cu = bpc;
  const long long tiles = doc_tiles(seg), slot_bytes = dma_slot_bytes(filter_bits, value_bits);
  k->dma_pair = g_engine.dma_pair != 0 && scan_simple_dma_pair_shape(filter_bits, value_bits);
  k->dma_nt = g_engine.dma_nt >= 0 ? g_engine.dma_nt == 1 : tiles * slot_bytes > kInfinityCacheBytes;
  const long long resident_waves = (long long)seg->num_cus * bpc * (kBlockThreads / 64);
  k->dma = g_engine.scan_simple_dma == 2 || (dense && slot_bytes >= kDmaMinSlotBytes && bpc >= kDmaBlocksPerCu && tiles >= kDmaMinTilesPerWave * resident_waves);
}
static ScanChoice choose_scan_kernel(const pg_segment* seg, const Lowered& lw, int hist_col, bool typed, bool want_bitmap, bool want_result) {
  const PlanParams& pl = lw.plan; const ScanParams& sp = lw.sp;
  const bool profile = (g_engine.flags & PG_CFG_PROFILE_WAVES) != 0;
  ScanChoice k;
  auto pick = [&k](ScanKernel kernel) { k.kernel = kernel; return k; };
  // A kLeafRawSet leaf exists only in a query lowered for scan_raw_set_kernel (raw_set_lean_shape: the shape test below for scan_raw_kernel,
  // applied to the query before its filter was lowered); no other kernel evaluates that kind.
  if (sp.num_nodes == 1 && sp.nodes[0].op == PG_FILTER_LEAF && sp.nodes[0].kind == kLeafRawSet) { k.general = ScanKernel::Private; return pick(ScanKernel::RawSet); }
  // The bitset pass of a DISTINCTCOUNT query: kernels of their own (pg_scan_distinct.h) with the lane-private filter -- check_distinct_plan
  // declined the leaves that filter does not evaluate.  Everything that goes by the family (tile lists, the entry counts) is Private's.
  // On raw columns both passes collect the values (pg_scan_collect.h).
  if (!lw.distinct_slots.empty() && lw.hll_pass) { k.general = ScanKernel::Private; return pick(lw.distinct_key_slots.empty() ? ScanKernel::Hll : ScanKernel::GroupHll); }      // DISTINCTCOUNTHLL on raw columns (pg_scan_hll.h)
  if (!lw.distinct_slots.empty() && lw.moments_pass) { k.general = ScanKernel::Private; return pick(lw.distinct_key_slots.empty() ? ScanKernel::Moments : ScanKernel::GroupMoments); }      // VARIANCE's moments (pg_scan_moments.h)
  if (!lw.distinct_slots.empty() && lw.collect_pass) { k.general = ScanKernel::Private; return pick(lw.distinct_key_slots.empty() ? ScanKernel::Collect : ScanKernel::GroupCollect); }
  if (!lw.distinct_slots.empty() && !lw.counts_pass) { k.general = ScanKernel::Private; return pick(lw.distinct_key_slots.empty() ? ScanKernel::Distinct : ScanKernel::GroupDistinct); }
  // The counts pass of a PERCENTILE query: the same, with 32-bit counters per dictId (pg_scan_counts.h).
  if (!lw.distinct_slots.empty()) { k.general = ScanKernel::Private; return pick(lw.distinct_key_slots.empty() ? ScanKernel::Counts : ScanKernel::GroupCounts); }
  // The lane-private kernel (no LDS, plain global loads) takes every query whose leaves and aggregations it implements:
  // scan / set / bitmap leaves and raw INT ranges; COUNT, and SUM through a value plane / MIN / MAX on dictionary columns.
  // (the per-wave phase counters of PG_CFG_PROFILE_WAVES exist in the LDS-staged kernel only)
  bool private_leaves = true;
  for (int l = 0; l < pl.num_leaves; ++l) private_leaves &= pl.leaves[l].kind <= kLeafBitmap || pl.leaves[l].kind == kLeafDocRange;
  bool lane_private = g_engine.scan_private && !typed && !profile && private_leaves;
  for (int i = 0; i < pl.num_agg_cols && hist_col >= 0; ++i) if (lw.col_of_slot[(size_t)pl.agg_cols[i].col] == hist_col * 2) k.hist_slot = i;
  for (int i = 0; i < pl.num_agg_cols && lane_private; ++i) {
    const DevColumn& c = pl.cols[pl.agg_cols[i].col];
    lane_private = !c.is_raw && c.vkind == kValI32 && c.bits <= 31 && (!pl.agg_cols[i].need_sum || c.is_plane || i == k.hist_slot);
  }
  const bool hist = lane_private && k.hist_slot == 0 && pl.num_agg_cols == 1;      // the histogram kernel aggregates one column
  if (k.hist_slot >= 0 && !hist) lane_private = false;                            // (rare: the gather path of the LDS-staged kernel)
  // Raw columns and 8-byte dictionaries: the same lane-private layout, read with 16-byte loads (scan_private_typed_kernel).
  // PINOT_GPU_SCAN_TYPED_PRIVATE=0 keeps them in the LDS-staged kernel.
  bool lane_typed = g_engine.scan_private && g_engine.scan_typed_private && !lane_private && pl.num_agg_cols > 0 && !profile && private_leaves;
  for (int i = 0; i < pl.num_agg_cols && lane_typed; ++i) {
    const DevColumn& c = pl.cols[pl.agg_cols[i].col];
    lane_typed = c.is_raw || (c.vkind != kValI32 && c.bits <= 31);      // every slot raw, or an 8-byte dictionary
  }
  k.general = k.kernel = lane_private ? ScanKernel::Private : (lane_typed ? ScanKernel::PrivateTyped : ScanKernel::Agg);
  if (hist) {
    k.hist_cw = hist_counter_bits(seg->cols[(size_t)hist_col]);
    k.hist_guarded = std::max(__atomic_load_n(&seg->cols[(size_t)hist_col].hist_tier, __ATOMIC_RELAXED), g_engine.hist_guard ? 1 : 0) >= 1 && k.hist_cw < 32;
    return pick(ScanKernel::Hist);
  }
  if (k.general == ScanKernel::Agg) return k;
  // Nothing but a filter over narrow dictionary columns (COUNT(*) and / or the bitmap): scan_narrow_kernel, four tiles per wave and iteration
  // (a leap-frogging `a AND b` is counted by eval_filter_private's hook: the narrow kernels have their own evaluator and do not carry it)
  if (g_engine.scan_narrow && lane_private && pl.num_agg_cols == 0 && lw.tile_list == nullptr && sp.num_nodes > 0 && !(want_result && lw.stats_leap2_flagged)) {
    bool narrow = true; int depth = 0, max_depth = 0;
    for (int n = 0; n < sp.num_nodes && narrow; ++n) {
      const DevNode& dn = sp.nodes[n];
      if (dn.op == PG_FILTER_LEAF) {
        narrow = dn.kind == kLeafMatchAll || dn.kind == kLeafMatchNone || ((dn.kind == kLeafDictRange || (dn.kind == kLeafDictSet && g_engine.set_lds)) && dn.bits >= 1 && dn.bits <= kNarrowMaxBits);      // (a set of a narrow column: eight words in LDS, pg_scan_narrow.h)
        depth++;
      } else if (dn.op != PG_FILTER_NOT) depth -= dn.num_children - 1;
      max_depth = std::max(max_depth, depth);
    }
    if (narrow && max_depth <= kNarrowStack)
      return pick(g_engine.scan_narrow_single && sp.num_nodes == 1 && sp.nodes[0].kind == kLeafDictRange ? ScanKernel::NarrowSingle : ScanKernel::Narrow);
  }
  // The whole filter is ONE bitmap that index_and_kernel made (its tiles listed), and every aggregated column is read as bit-packed
  // fields: eight tiles per wave and iteration, only the matching docs' values are touched (scan_sparse_kernel)
  if (g_engine.scan_sparse && lane_private && !want_bitmap && pl.num_agg_cols > 0 && lw.tile_list != nullptr && sp.num_nodes == 1 && sp.nodes[0].kind == kLeafBitmap &&
      sp.nodes[0].exclusive == 0) return pick(ScanKernel::Sparse);
  // The queryable docIds of an upsert / dedup segment in front of scan_simple_kernel's shape: a root AND of ONE non-exclusive doc-set leaf
  // (first in the chain: bitmap leaves lead) and at most one dictionary-range leaf, or the doc set alone, and at most one aggregated packed
  // column, widths up to kSimpleMaxBits -- scan_simple_valid_kernel.  The chain's entry count is a closed form there (one entry per doc of
  // the set: run_aggregation), so stats_chain_flagged does not keep the query out.
  if (g_engine.scan_simple_valid != 0 && g_engine.scan_simple && lane_private && !want_bitmap && lw.tile_list == nullptr && lw.side == nullptr && lw.valid_leaf >= 0 &&
      pl.num_agg_cols <= 1 && !lw.stats_leap2_flagged && (sp.num_nodes == 1 || sp.num_nodes == 3)) {
    const DevNode& v = sp.nodes[0];
    const DevNode* range = sp.num_nodes == 3 ? &sp.nodes[1] : nullptr;
    const DevAggCol* vac = pl.num_agg_cols == 1 ? &sp.agg_cols[0] : nullptr;
    bool valid = v.op == PG_FILTER_LEAF && v.kind == kLeafBitmap && v.exclusive == 0 && v.set_words == reinterpret_cast<const uint32_t*>(pl.leaves[lw.valid_leaf].bitmap) &&
                 (range != nullptr || vac != nullptr);
    if (valid && range != nullptr)
      valid = sp.nodes[2].op == PG_FILTER_AND && sp.nodes[2].num_children == 2 && range->op == PG_FILTER_LEAF && range->kind == kLeafDictRange && range->bits >= 1 && range->bits <= kSimpleMaxBits &&
              (range->flags & kNodeLeapfrog2) == 0;
    if (valid && vac != nullptr)
      valid = vac->bits >= 1 && vac->bits <= kSimpleMaxBits && !vac->is_raw &&
              !(range != nullptr && range->fwd == vac->fwd && range->bits == vac->bits && vac->need_sum != 0 && vac->need_minmax == 0 && range->exclusive == 0);
    if (valid) return pick(ScanKernel::SimpleValid);
  }
  // the lean kernels below: at most one leaf (without the count hooks) and one aggregated column, no tile list, no statistics they do not count
  if (want_bitmap || lw.tile_list != nullptr || sp.num_nodes > 1 || pl.num_agg_cols > 1 || (want_result && (lw.stats_leap2_flagged || lw.stats_chain_flagged))) return k;
  const DevNode* leaf = sp.num_nodes == 1 ? &sp.nodes[0] : nullptr;
  const bool plain_leaf = leaf == nullptr || (leaf->op == PG_FILTER_LEAF && (leaf->flags & (kNodeCountEntries | kNodeLeapfrog2)) == 0);
  const DevAggCol* ac = pl.num_agg_cols == 1 ? &sp.agg_cols[0] : nullptr;
  // One dictionary-range leaf (or no filter) in front of at most one aggregated packed column, both of at most kSimpleMaxBits bits:
  // scan_simple_kernel -- the same per-tile code with none of the general machinery, at twice the waves per SIMD (pg_scan_simple.h).
  // (the one-stream shape `SUM(v) WHERE v in range` keeps scan_private_kernel's fused decode)
  // (a dictId SET over a column of at most 16 bits -- its words fit the LDS area -- takes scan_simple_set_kernel: round 6b)
  const bool set = leaf != nullptr && leaf->op == PG_FILTER_LEAF && leaf->kind == kLeafDictSet && g_engine.set_lds && leaf->bits <= 16;
  bool simple = g_engine.scan_simple && lane_private && plain_leaf &&
                (leaf == nullptr || ((leaf->kind == kLeafDictRange || set) && leaf->bits >= 1 && leaf->bits <= kSimpleMaxBits));
  if (simple && ac != nullptr)
    simple = ac->bits >= 1 && ac->bits <= kSimpleMaxBits && !ac->is_raw && !(leaf != nullptr && leaf->fwd == ac->fwd && leaf->bits == ac->bits && ac->need_sum != 0 && ac->need_minmax == 0 && leaf->exclusive == 0);
  if (simple && !set && leaf != nullptr && leaf->kind == kLeafDictRange && ac != nullptr) {
    const DevColumn& fc = pl.cols[pl.leaves[pl.nodes[0].leaf].col];
    const unsigned long long values = fc.is_plane ? 1ull << leaf->bits : (unsigned long long)std::max(fc.cardinality, 1);      // (a range over a value plane: span is in plane units)
    const unsigned long long inside = std::min<unsigned long long>(leaf->span, values), taken = leaf->exclusive ? values - inside : inside;
    const bool dense = taken * 100ull >= (unsigned long long)kPipeMinSelectivityPct * values;
    if (g_engine.scan_simple_pipe != 0 && scan_simple_pipe_shape(leaf->bits, ac->bits)) k.pipe = g_engine.scan_simple_pipe == 2 || dense;
    if (g_engine.scan_simple_dma != 0) plan_scan_simple_dma(seg, leaf->bits, ac->bits, dense, &k);
  }
  if (simple) return pick(set ? ScanKernel::SimpleSet : ScanKernel::Simple);
  // The same idea for raw INT columns (BASELINE.json configs[0]'s scan pair): one raw-range leaf (or no filter) in front of at most one
  // aggregated raw INT column -- scan_raw_kernel, five waves per SIMD, coalesced reads (pg_scan_raw.h).
  if (g_engine.scan_raw && lw.side == nullptr && sp.num_nodes + pl.num_agg_cols >= 1 && plain_leaf && (leaf == nullptr || (leaf->kind == kLeafRawRange && leaf->fwd != nullptr)) &&
      (ac == nullptr || (ac->is_raw != 0 && ac->vkind == kValI32 && ac->is_plane == 0 && ac->bits == 32))) return pick(ScanKernel::Raw);
  return k;
}
// threads: the workgroup the kernel's records are counted in (profile_waves); lds: Agg's staged layout, or Hist's histogram with the set
// area at hist_set_off; wide: scan_simple / scan_raw launch workgroups of kWideBlockThreads (PINOT_GPU_WIDE_BLOCKS=1)
// scan_counts_kernel's LDS tier: the reduction records of a workgroup of kHistBlockThreads, and the counters that fit beside them without a staged set
constexpr size_t kCountsRecordBytes = sizeof(BlockPartial) * (kHistBlockThreads / 64) + 16;
static_assert((kLdsBudget - kCountsRecordBytes) / 4 == PG_PERCENTILE_LDS_MAX_COUNTERS, "include/pinot_gpu.h states the LDS tier's reach");
// scan_distinct_kernel's LDS tier: the reduction records overlay the bitsets' start (the maximum, not the sum, is the rule), so the whole budget holds bits
static_assert(kLdsBudget * 8 == PG_DISTINCT_LDS_MAX_DICT_IDS, "include/pinot_gpu.h states the LDS tier's reach");
static_assert(kSetLdsWords == PG_STAGED_SET_LDS_WORDS, "include/pinot_gpu.h states the staged set area");
// distinct_lds: scan_distinct_kernel / scan_counts_kernel keep their bitsets / counters in LDS (the set passes' parameter blocks and launches: SetPass, below)
struct ScanGrid { int blocks = 1, threads = kBlockThreads; size_t lds = 0, hist_set_off = 0; bool wide = false, distinct_lds = false; };
// A segment whose tiles all fit the chip at once (one tile per wave: a 10 M-row segment at five waves per SIMD) is latency from end
// to end -- launch, one round of loads, the hand-off of the workgroups' records to the fold.  Ten waves per workgroup there: 2.5x
// fewer records, and a folding workgroup of 640 threads takes them in ONE round of loads (256 threads took five for 1221 records).
static void lean_grid(const pg_segment* seg, int wave_cap, ScanGrid* g) {
  const long long tiles2k = doc_tiles(seg);
  static const bool wide_ok = getenv("PINOT_GPU_WIDE_BLOCKS") && getenv("PINOT_GPU_WIDE_BLOCKS")[0] == '1';      // (measured slower at every size: off unless asked for)
  g->wide = wide_ok && wave_cap >= 2 * (kWideBlockThreads / 64) && tiles2k > 64 && tiles2k <= (long long)seg->num_cus * wave_cap && g_engine.blocks_per_cu <= 0;
  const int wpb = (g->wide ? kWideBlockThreads : kBlockThreads) / 64;
  int bpc = std::max(1, wave_cap / wpb);
  // Up to two rounds of resident waves' worth of tiles (~20 M rows), the hand-off of the workgroups' records to the fold weighs more
  // than a second round of loads: two workgroups per CU (profiles/r4/c1_probe_blocks_per_cu.jsonl: 10 M rows, 1221 workgroups
  // 21.4 us, 512 workgroups 17.8 us; the scan alone 12.9 us)
  static const int small_bpc = getenv("PINOT_GPU_SMALL_BLOCKS_PER_CU") ? atoi(getenv("PINOT_GPU_SMALL_BLOCKS_PER_CU")) : 2;
  if (!g->wide && small_bpc > 0 && tiles2k <= 2ll * seg->num_cus * wave_cap) bpc = std::min(bpc, small_bpc);
  g->blocks = grid_blocks(seg, tiles2k, wpb, bpc);
}
// The chosen kernel's grid (`geo`: the layout finish_geometry made for the LDS-staged kernel).  PrivateFsm is chosen after the grid: Private's.
static ScanGrid scan_grid(const pg_segment* seg, const ScanChoice& k, const Lowered& lw, const Geometry& geo, int num_agg_cols, int hist_col) {
  const ScanParams& sp = lw.sp;
  ScanGrid g;
  const long long tiles = doc_tiles(seg);
  const int wpb = kBlockThreads / 64, hist_waves = kHistBlockThreads / 64;
  switch (k.kernel) {
    case ScanKernel::Hist: {
      // one histogram per workgroup of 16 wavefronts; as many workgroups per CU as LDS and registers admit
      const int per_word = 32 / k.hist_cw;
      g.lds = (((size_t)(seg->cols[(size_t)hist_col].cardinality + per_word - 1) / per_word * 4) + 15) & ~(size_t)15;
      g.lds = std::max(g.lds, sizeof(BlockPartial) * (kHistBlockThreads / 64) + 16);      // the reduction records (+ the fold flag) reuse the counters' LDS
      // the filter's dictId sets (IN lists) behind the counters: ScanParams.set_leaves_in_lds = 1 + the area's byte offset (scan_hist_body)
      if (g_engine.set_lds && g.lds + (size_t)kSetLdsWords * 4 <= 150 * 1024)
        for (int nd = 0; nd < sp.num_nodes; ++nd) if (sp.nodes[nd].op == PG_FILTER_LEAF && sp.nodes[nd].kind == kLeafDictSet) g.hist_set_off = g.lds;
      if (g.hist_set_off != 0) g.lds += (size_t)kSetLdsWords * 4;
      g.threads = kHistBlockThreads;
      g.blocks = grid_blocks(seg, tiles, hist_waves, std::max(1, std::min(waves_scan_hist(k.hist_cw, k.hist_guarded) / hist_waves, (int)((160 * 1024 - 2048) / (g.lds + 256)))));
      if (g_engine.hist_blocks > 0) g.blocks = std::min(g.blocks, g_engine.hist_blocks);
      break;
    }
    case ScanKernel::Distinct: case ScanKernel::GroupDistinct: {
      // LDS tier: the columns' bitsets side by side, the filter's set area behind them, the reduction records over their start at the end -- one
      // bitset per workgroup of 16 wavefronts, as many workgroups per CU as LDS and registers admit (the Hist case's sizing).  Else the bitsets
      // stay in HBM: workgroups of four wavefronts, the set area (if any) 16 bytes in (set_leaves_in_lds = 1 + offset must exceed 1).
      bool has_set = false;
      if (g_engine.set_lds) for (int nd = 0; nd < sp.num_nodes; ++nd) has_set |= sp.nodes[nd].op == PG_FILTER_LEAF && sp.nodes[nd].kind == kLeafDictSet;
      size_t bit_bytes = 0;
      for (int slot : lw.distinct_slots) bit_bytes += (size_t)((lw.plan.cols[slot].cardinality + 31) / 32) * 4;
      bit_bytes = (bit_bytes + 15) & ~(size_t)15;
      const size_t records = sizeof(BlockPartial) * (kHistBlockThreads / 64) + 16;
      size_t lds_tier = bit_bytes + (has_set ? (size_t)kSetLdsWords * 4 : 0);
      if (lds_tier > kLdsBudget && bit_bytes <= kLdsBudget) { has_set = false; lds_tier = bit_bytes; }      // (the sets stay in memory rather than push the bitsets out)
      g.distinct_lds = k.kernel == ScanKernel::Distinct && g_engine.distinct_lds && std::max(lds_tier, records) <= kLdsBudget;
      if (g.distinct_lds) {
        g.hist_set_off = has_set ? bit_bytes : 0;
        g.lds = std::max(lds_tier, records);
        g.threads = kHistBlockThreads;
        g.blocks = grid_blocks(seg, tiles, hist_waves, std::max(1, std::min(waves_scan_distinct(true) / hist_waves, (int)((160 * 1024 - 2048) / (g.lds + 256)))));
      } else {
        g.hist_set_off = has_set ? 16 : 0;
        g.lds = std::max((size_t)(has_set ? 16 + kSetLdsWords * 4 : 0), sizeof(BlockPartial) * (size_t)wpb + 16);
        g.blocks = grid_blocks(seg, tiles, wpb, std::max(1, (k.kernel == ScanKernel::Distinct ? waves_scan_distinct(false) : waves_group_distinct()) / wpb));
      }
      break;
    }
    case ScanKernel::Counts: case ScanKernel::GroupCounts: {
      // The Distinct case with 32-bit counters.  LDS tier: the columns' counters side by side, the filter's set area behind them; it applies while
      // counters + set area + the reduction records fit kLdsBudget (the records overlay the counters' start once the workgroup has flushed them:
      // the sum, not the maximum, is the rule -- PG_PERCENTILE_LDS_MAX_COUNTERS states it for a filter without a staged set).
      bool has_set = false;
      if (g_engine.set_lds) for (int nd = 0; nd < sp.num_nodes; ++nd) has_set |= sp.nodes[nd].op == PG_FILTER_LEAF && sp.nodes[nd].kind == kLeafDictSet;
      size_t counter_bytes = 0;
      for (int slot : lw.distinct_slots) counter_bytes += (size_t)std::max(lw.plan.cols[slot].cardinality, 0) * 4;
      counter_bytes = (counter_bytes + 15) & ~(size_t)15;
      size_t lds_tier = counter_bytes + (has_set ? (size_t)kSetLdsWords * 4 : 0);
      if (lds_tier + kCountsRecordBytes > kLdsBudget && counter_bytes + kCountsRecordBytes <= kLdsBudget) { has_set = false; lds_tier = counter_bytes; }      // (the sets stay in memory rather than push the counters out)
      g.distinct_lds = k.kernel == ScanKernel::Counts && g_engine.percentile_lds && lds_tier + kCountsRecordBytes <= kLdsBudget;
      if (g.distinct_lds) {
        g.hist_set_off = has_set ? counter_bytes : 0;
        g.lds = std::max(lds_tier, kCountsRecordBytes);
        g.threads = kHistBlockThreads;
        g.blocks = grid_blocks(seg, tiles, hist_waves, std::max(1, std::min(waves_scan_counts(true) / hist_waves, (int)((160 * 1024 - 2048) / (g.lds + 256)))));
      } else {
        g.hist_set_off = has_set ? 16 : 0;
        g.lds = std::max((size_t)(has_set ? 16 + kSetLdsWords * 4 : 0), sizeof(BlockPartial) * (size_t)wpb + 16);
        g.blocks = grid_blocks(seg, tiles, wpb, std::max(1, (k.kernel == ScanKernel::Counts ? waves_scan_counts(false) : waves_group_counts()) / wpb));
      }
      break;
    }
    case ScanKernel::Collect: case ScanKernel::GroupCollect: {
      // the HBM tier of the two cases above: workgroups of four wavefronts, the filter's set area (if any) 16 bytes in, the reduction records over the start
      bool has_set = false;
      if (g_engine.set_lds) for (int nd = 0; nd < sp.num_nodes; ++nd) has_set |= sp.nodes[nd].op == PG_FILTER_LEAF && sp.nodes[nd].kind == kLeafDictSet;
      g.hist_set_off = has_set ? 16 : 0;
      g.lds = std::max((size_t)(has_set ? 16 + kSetLdsWords * 4 : 0), sizeof(BlockPartial) * (size_t)wpb + 16);
      g.blocks = grid_blocks(seg, tiles, wpb, std::max(1, (k.kernel == ScanKernel::Collect ? waves_scan_collect() : waves_group_collect()) / wpb));
      break;
    }
    case ScanKernel::Hll: {
      // every slot's registers side by side, the filter's set area behind them, the reduction records over their start at the end -- one register set
      // per workgroup of 16 wavefronts (the Distinct case's LDS tier; plan_distinct priced registers + set area against kLdsBudget and declined
      // what does not fit: there is no HBM tier and no fallback here)
      bool has_set = false;
      if (g_engine.set_lds) for (int nd = 0; nd < sp.num_nodes; ++nd) has_set |= sp.nodes[nd].op == PG_FILTER_LEAF && sp.nodes[nd].kind == kLeafDictSet;
      size_t reg_bytes = 0;
      for (int log2m : lw.hll_slot_log2m) reg_bytes += (size_t)4 << log2m;
      g.hist_set_off = has_set ? reg_bytes : 0;
      g.lds = std::max(reg_bytes + (has_set ? (size_t)kSetLdsWords * 4 : 0), kCountsRecordBytes);
      g.threads = kHistBlockThreads;
      g.blocks = grid_blocks(seg, tiles, hist_waves, std::max(1, std::min(waves_scan_hll() / hist_waves, (int)((160 * 1024 - 2048) / (g.lds + 256)))));
      break;
    }
    case ScanKernel::GroupHll: {
      // the matrices live in HBM: workgroups of four wavefronts, the filter's set area (if any) 16 bytes in, the reduction records over the start
      bool has_set = false;
      if (g_engine.set_lds) for (int nd = 0; nd < sp.num_nodes; ++nd) has_set |= sp.nodes[nd].op == PG_FILTER_LEAF && sp.nodes[nd].kind == kLeafDictSet;
      g.hist_set_off = has_set ? 16 : 0;
      g.lds = std::max((size_t)(has_set ? 16 + kSetLdsWords * 4 : 0), sizeof(BlockPartial) * (size_t)wpb + 16);
      g.blocks = grid_blocks(seg, tiles, wpb, std::max(1, waves_group_hll() / wpb));
      break;
    }
    case ScanKernel::Moments: case ScanKernel::GroupMoments: {
      // the accumulators live in registers (the matrices in HBM): workgroups of four wavefronts, the filter's set area (if any) 16 bytes in, the
      // wavefronts' sums and then the reduction records over the start
      bool has_set = false;
      if (g_engine.set_lds) for (int nd = 0; nd < sp.num_nodes; ++nd) has_set |= sp.nodes[nd].op == PG_FILTER_LEAF && sp.nodes[nd].kind == kLeafDictSet;
      g.hist_set_off = has_set ? 16 : 0;
      g.lds = std::max((size_t)(has_set ? 16 + kSetLdsWords * 4 : 0), sizeof(BlockPartial) * (size_t)wpb + 16);
      g.blocks = grid_blocks(seg, tiles, wpb, std::max(1, (k.kernel == ScanKernel::Moments ? waves_scan_moments() : waves_group_moments()) / wpb));
      break;
    }
    case ScanKernel::Narrow: g.blocks = grid_blocks(seg, (tiles + kNarrowTiles - 1) / kNarrowTiles, wpb, std::max(1, waves_scan_narrow(false) / wpb)); break;
    case ScanKernel::NarrowSingle: g.blocks = grid_blocks(seg, (tiles + kNarrowSingleTiles - 1) / kNarrowSingleTiles, wpb, std::max(1, waves_scan_narrow(true) / wpb)); break;
    case ScanKernel::Sparse: g.blocks = grid_blocks(seg, tiles, wpb * kSparseTiles, std::max(1, waves_scan_sparse(num_agg_cols <= 1) / wpb)); break;
    case ScanKernel::Simple: case ScanKernel::SimpleSet:
      if (k.dma) {
        // the rings are dynamic LDS: the workgroups per CU are those plan_scan_simple_dma found room for; small grids as lean_grid
        g.lds = scan_simple_dma_lds(sp.nodes[0].bits, sp.agg_cols[0].bits);
        g.blocks = grid_blocks(seg, tiles, wpb, k.dma_blocks_per_cu, false);
      } else lean_grid(seg, k.pipe ? waves_scan_simple_pipe() : waves_scan_simple(), &g);
      break;
    case ScanKernel::SimpleValid: lean_grid(seg, waves_scan_simple_valid(), &g); break;
    case ScanKernel::Raw: lean_grid(seg, waves_scan_raw(), &g); break;
    case ScanKernel::RawSet: {
      // every workgroup keeps the leaf's table in dynamic LDS: as many workgroups per CU as registers AND the tables admit; small grids two, as lean_grid
      g.lds = (size_t)sp.nodes[0].set_bytes;
      int bpc = std::max(1, std::min(waves_scan_raw_set(sp.nodes[0].lo_hi) / wpb, (int)(kLdsBudget / (g.lds + 1024))));
      if (tiles <= 2ll * seg->num_cus * bpc * wpb) bpc = std::min(bpc, 2);
      g.blocks = grid_blocks(seg, tiles, wpb, bpc);
      break;
    }
    case ScanKernel::Private: g.blocks = grid_blocks(seg, tiles, wpb, std::max(1, waves_scan_private(num_agg_cols) / wpb)); break;
    case ScanKernel::PrivateTyped: g.blocks = grid_blocks(seg, tiles, wpb, std::max(1, waves_scan_private_typed(num_agg_cols) / wpb)); break;
    default: g.blocks = geo.blocks; g.threads = geo.threads; g.lds = geo.lds; break;      // Agg
  }
  return g;
}
// The kind of shared launch an item of the chosen kernel joins (false: none, it runs its own kernel).  Without PINOT_GPU_LEAN_BATCH the
// simple shapes join the general kind; a raw-shaped item has no general form when its column is aggregated: it stays lean.
static bool scan_batch_kind(const ScanChoice& k, int num_agg_cols, BatchKind* kind) {
  const bool lean = g_engine.lean_batch;
  switch (k.kernel) {
    case ScanKernel::Hist: *kind = k.hist_cw == 8 ? BatchKind::Hist8 : (k.hist_cw == 16 ? BatchKind::Hist16 : BatchKind::Hist32); return !k.hist_guarded && g_engine.batch_hist;
    case ScanKernel::Narrow: case ScanKernel::NarrowSingle: *kind = k.kernel == ScanKernel::Narrow ? BatchKind::Narrow : BatchKind::NarrowSingle; return g_engine.batch_more;
    case ScanKernel::Simple: case ScanKernel::SimpleSet: *kind = !lean ? BatchKind::Private : (k.kernel == ScanKernel::Simple ? BatchKind::Simple : BatchKind::SimpleSet); return true;
    case ScanKernel::Raw: *kind = !lean && k.general == ScanKernel::Private ? BatchKind::Private : BatchKind::Raw; return true;
    case ScanKernel::RawSet: return false;      // (no shared-launch form: the table belongs to the context)
    case ScanKernel::SimpleValid: return false; // (no shared-launch form: a batch item behind a doc set runs its own kernel)
    case ScanKernel::PrivateFsm: case ScanKernel::Private: *kind = BatchKind::Private; return true;
    case ScanKernel::PrivateTyped: *kind = num_agg_cols <= 1 ? BatchKind::Typed1 : (num_agg_cols == 2 ? BatchKind::Typed2 : BatchKind::TypedMax); return g_engine.batch_more;
    default: return false;      // Sparse, Agg
  }
}
static void launch_scan_kernel(const ScanChoice& k, const ScanGrid& g, int num_agg_cols, bool typed, hipStream_t stream, const ScanParams& sp) {
  const bool one = num_agg_cols <= 1;      // the single-aggregated-column instantiation needs a third fewer registers (one more wavefront per SIMD)
  const int lean_threads = g.wide ? kWideBlockThreads : kBlockThreads;
  switch (k.kernel) {
    case ScanKernel::Hist: launch_scan_hist(k.hist_cw, k.hist_guarded, g.blocks, g.lds, stream, sp); break;
    case ScanKernel::Narrow: case ScanKernel::NarrowSingle: launch_scan_narrow(k.kernel == ScanKernel::NarrowSingle, g.blocks, stream, sp); break;
    case ScanKernel::Sparse: launch_scan_sparse(one, g.blocks, stream, sp); break;
    case ScanKernel::Simple: case ScanKernel::SimpleSet:
      if (k.dma) launch_scan_simple_dma(g.blocks, k.dma_nt, k.dma_pair, stream, sp);
      else if (k.pipe) launch_scan_simple_pipe(g.blocks, lean_threads, stream, sp);
      else launch_scan_simple(g.blocks, lean_threads, stream, sp, k.kernel == ScanKernel::SimpleSet);
      break;
    case ScanKernel::SimpleValid: launch_scan_simple_valid(g.blocks, lean_threads, stream, sp, g_engine.scan_simple_valid == 2); break;
    case ScanKernel::Raw: launch_scan_raw(g.blocks, lean_threads, stream, sp); break;
    case ScanKernel::RawSet: launch_scan_raw_set(sp.nodes[0].lo_hi, g.blocks, g.lds, stream, sp); break;
    case ScanKernel::PrivateFsm: launch_scan_private_fsm(num_agg_cols, g.blocks, stream, sp); break;
    case ScanKernel::Private: launch_scan_private(num_agg_cols, g.blocks, stream, sp); break;
    case ScanKernel::PrivateTyped: launch_scan_private_typed(num_agg_cols, g.blocks, stream, sp); break;
    case ScanKernel::Agg: launch_scan_agg(g_engine.use_dma, one, typed, g.blocks, g.threads, g.lds, stream, sp); break;
    case ScanKernel::Distinct: case ScanKernel::GroupDistinct: case ScanKernel::Counts: case ScanKernel::GroupCounts:
    case ScanKernel::Collect: case ScanKernel::GroupCollect: case ScanKernel::Hll: case ScanKernel::GroupHll: case ScanKernel::Moments: case ScanKernel::GroupMoments: break;      // (launched with their own parameter block: launch_set_pass)
  }
}
// What the phases of execute_impl share about one query
struct QueryRun {
  pg_segment* seg; const pg_query* q; pg_result* out; ExecCtx* ctx; Deferred* defer;
  int na, ng, hist_col = -1;          // hist_col: the summed column that goes through the LDS histogram (scan_hist_kernel)
  bool want_bitmap, timed, stats_is_final = false;
  Lowered lw;
  PlaneHold planes;                   // the value planes the kernels read
  std::vector<int> projected;         // distinct projected columns (ExecutionStatistics numEntriesScannedPostFilter = numDocsScanned * numProjectedColumns)
  QueryRun(pg_segment* s, const pg_query* q_, pg_result* o, ExecCtx* c, Deferred* d, int na_, int ng_, bool want_bitmap_, bool timed_)
      : seg(s), q(q_), out(o), ctx(c), defer(d), na(na_), ng(ng_), want_bitmap(want_bitmap_), timed(timed_), planes(s, {}) {}
  void add_projected(int c) { if (std::find(projected.begin(), projected.end(), c) == projected.end()) projected.push_back(c); }
};
// The query becomes an item of pg_execute_batch's shared launch; the value planes its kernel reads stay held until the batch has run
static pg_status defer_item(QueryRun& r, std::shared_ptr<LoweredItem> item) {
  item->plane_columns = r.planes.columns;      // (none for an index-only COUNT)
  item->doc_sets = r.lw.doc_sets;
  r.defer->item = std::move(item);
  r.defer->cacheable = !r.lw.plane_pending;
  r.defer->planes.reset(new PlaneHold(std::move(r.planes)));
  return kDeferred;
}
// an item whose whole device work is index_and_kernel publishing the query's record (BatchKind::IndexAnd)
static std::shared_ptr<LoweredItem> index_and_item(const Lowered& lw) {
  auto item = std::make_shared<LoweredItem>();
  memset(&item->sp, 0, sizeof(item->sp));
  item->sp.lean_kind = (int32_t)BatchKind::IndexAnd;
  item->and_params = std::make_shared<IndexAndParams>(lw.and_params);
  item->and_windows = lw.finalize_windows;
  item->blocks = (int)std::min<long long>(((long long)lw.finalize_windows + index_and_batch_block_waves() - 1) / index_and_batch_block_waves(), (long long)lw.and_num_cus * index_and_batch_blocks_per_cu());
  return item;
}
// a holder that no value reached yet; the statistics of an answer that scanned nothing
static void empty_agg_value(pg_agg_value* v, int64_t count) { v->count = count; v->min = std::numeric_limits<double>::infinity(); v->max = -std::numeric_limits<double>::infinity(); }
// index_and_kernel is the query: [ev[0], ev[3]] brackets the kernel and the copy of its counter lines
static void nothing_scanned(pg_result* o, int64_t docs, int total_docs) {
  o->stats.num_docs_scanned = docs; o->stats.num_entries_scanned_in_filter = 0; o->filter_entries_exact = 1; o->stats.num_entries_scanned_post_filter = 0; o->stats.num_total_docs = total_docs;
}
// a group-by result's header and its arrays for num_present groups (pg_result_free releases them)
static void start_group_result(pg_result* out, int na, int ng, int num_present, int kernel, int upper_bound, int key_kind) {
  out->num_aggregations = na; out->dominant_kernel = kernel; out->num_groups = num_present; out->group_id_upper_bound = upper_bound;
  out->group_ids = (int32_t*)malloc(sizeof(int32_t) * (size_t)std::max(num_present, 1));
  out->group_aggregations = (pg_agg_value*)calloc((size_t)std::max(num_present, 1) * (size_t)std::max(na, 1), sizeof(pg_agg_value));
  out->group_key_dict_ids = (int32_t*)malloc(sizeof(int32_t) * (size_t)std::max(num_present, 1) * (size_t)ng);
  out->group_key_kind = key_kind;
}
static pg_status time_index_and(const ExecCtx* ctx, pg_result* out) {
  float ms_all = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms_all, ctx->ev[0], ctx->ev[3]));
  out->device_ms = ms_all; out->dominant_kernel_ms = ms_all;
  return PG_OK;
}
// NonScanBasedAggregationOperator (core/plan/AggregationPlanNode.java:98-115,159-190; core/operator/query/
// NonScanBasedAggregationOperator.java:83-105): the filter matches everything and every function is COUNT, or MIN / MAX of a
// dictionary column -> the answer comes from the segment metadata and the dictionary ends; nothing is scanned.
static bool answer_from_metadata(const pg_segment* seg, const pg_query* q, int na, pg_result* out, int64_t* out_cardinality) {
  bool match_all = q->num_filter_nodes == 0;
  if (q->num_filter_nodes == 1 && q->filter && q->predicates && q->filter[0].op == PG_FILTER_LEAF && q->filter[0].predicate >= 0 &&
      q->filter[0].predicate < q->num_predicates) {
    const pg_predicate& pr = q->predicates[q->filter[0].predicate];
    match_all = (pr.kind == PG_PRED_MATCH_ALL && !pr.exclusive) || (pr.kind == PG_PRED_MATCH_NONE && pr.exclusive);
  }
  bool fit = match_all;
  for (int a = 0; a < na && fit; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    if (ag.function == PG_AGG_COUNT) continue;
    fit = (ag.function == PG_AGG_MIN || ag.function == PG_AGG_MAX) && ag.column >= 0 && ag.column < (int)seg->cols.size() &&
          seg->cols[(size_t)ag.column].encoding == PG_FWD_FIXED_BIT_DICT;
  }
  if (!fit) return false;
  memset(out, 0, sizeof(*out));
  out->num_aggregations = na;
  out->aggregations = (pg_agg_value*)calloc((size_t)na, sizeof(pg_agg_value));
  for (int a = 0; a < na; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    pg_agg_value& v = out->aggregations[a];
    empty_agg_value(&v, seg->num_docs);
    if (ag.function == PG_AGG_MIN) v.min = seg->cols[(size_t)ag.column].h_dict_f64.front();
    if (ag.function == PG_AGG_MAX) v.max = seg->cols[(size_t)ag.column].h_dict_f64.back();
  }
  nothing_scanned(out, seg->num_docs, seg->num_docs);      // NonScanBasedAggregationOperator.getExecutionStatistics: (totalDocs, 0, 0, totalDocs)
  if (out_cardinality) *out_cardinality = seg->num_docs;
  return true;
}
// FastFilteredCountOperator over the queryable docIds alone (COUNT(*) on an upsert segment without a user filter): the doc set's
// cardinality was computed when it was created -- nothing is launched.  Statistics (cardinality, 0, 0, totalDocs).
static bool answer_from_doc_set(const pg_segment* seg, const pg_query* q, int na, pg_result* out, int64_t* out_cardinality) {
  if (q->num_filter_nodes != 1 || !q->filter || !q->predicates || q->filter[0].op != PG_FILTER_LEAF || q->filter[0].predicate < 0 || q->filter[0].predicate >= q->num_predicates) return false;
  const pg_predicate& pr = q->predicates[q->filter[0].predicate];
  if (pr.kind != PG_PRED_DOC_SET) return false;
  for (int a = 0; a < na; ++a) if (q->aggregations[a].function != PG_AGG_COUNT || ((q->flags & kQueryCountReadsColumn) && q->aggregations[a].column >= 0)) return false;
  const std::shared_ptr<DocSet> ds = find_doc_set(seg, pr.lo);
  if (!ds) return false;                              // (the lowering reports the unknown id)
  const int64_t card = pr.exclusive ? (int64_t)seg->num_docs - ds->cardinality : ds->cardinality;
  memset(out, 0, sizeof(*out));
  out->num_aggregations = na;
  out->aggregations = (pg_agg_value*)calloc((size_t)na, sizeof(pg_agg_value));
  for (int a = 0; a < na; ++a) empty_agg_value(&out->aggregations[a], card);
  out->dominant_kernel = PG_KERNEL_INDEX_AND;
  nothing_scanned(out, card, seg->num_docs);
  if (out_cardinality) *out_cardinality = card;
  return true;
}
// FastFilteredCountOperator (core/plan/AggregationPlanNode.java:98-115, core/operator/query/FastFilteredCountOperator.java:66-72): COUNT(*)
// over a filter that the indexes answer alone is the cardinality of the and-ed bitmaps -- index_and_kernel counted it, nothing is scanned.
static pg_status count_from_index(QueryRun& r, int64_t* out_cardinality) {
  pg_segment* seg = r.seg; pg_result* out = r.out; ExecCtx* ctx = r.ctx; Lowered& lw = r.lw; const int na = r.na; const bool timed = r.timed;
  pg_status st = PG_OK;
  const int total_docs = seg->num_docs;
  auto convert = [na, total_docs](const BlockPartial& fp, pg_result* o) {
    const int64_t card = (int64_t)fp.count;
    o->num_aggregations = na;
    o->aggregations = (pg_agg_value*)calloc((size_t)na, sizeof(pg_agg_value));
    for (int a = 0; a < na; ++a) empty_agg_value(&o->aggregations[a], card);
    o->dominant_kernel = PG_KERNEL_INDEX_AND;
    nothing_scanned(o, card, total_docs);     // bitmaps only: nothing is scanned
  };
  if (r.defer != nullptr && !r.defer->single && g_engine.batch_index && g_engine.direct_result && lw.and_cardinality_only && index_and_shares_a_launch(lw)) {
    // pg_execute_batch: the item is index_and_kernel publishing the cardinality -- it shares index_and_batch_kernel's launch (BatchKind::IndexAnd)
    auto item = index_and_item(lw);
    item->convert = convert;
    return defer_item(r, std::move(item));
  }
  st = launch_index_and(&lw, ctx, nullptr); if (st != PG_OK) return st;
  unsigned long long* h_card = &ctx->h_partial->count;
  if (lw.cardinality_atomic) HIP_TRY(hipMemcpyAsync(ctx->h_and_shards, ctx->d_and_counters + 2, kAndShardBytes, hipMemcpyDeviceToHost, ctx->stream));
  else HIP_TRY(hipMemcpyAsync(h_card, lw.d_cardinality, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (timed) { HIP_TRY(mark_pre_work(ctx)); HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream)); }
  exec_mark(3);
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  exec_mark(4);
  if (lw.cardinality_atomic) {
    BlockPartial g;
    st = read_index_and_shards(ctx, 0, &g); if (st != PG_OK) return st;
    *h_card = g.count;
  }
  convert(*ctx->h_partial, out);      // (h_card is its count)
  if (out_cardinality) *out_cardinality = (int64_t)*h_card;
  return timed ? time_index_and(ctx, out) : PG_OK;
}
// ---- DISTINCTCOUNTHLL (pg_scan_hll.h): helpers of the two passes ----
static int64_t hll_nonzero(const uint8_t* registers, size_t n) { int64_t c = 0; for (size_t j = 0; j < n; ++j) c += registers[j] != 0; return c; }
// rows << log2m packed registers, from byte `first` of the pass's host copy
static HllSet hll_set_of(const std::vector<uint8_t>& host, size_t first, int aggregation, int log2m, long long rows) {
  HllSet hs;
  hs.aggregation = aggregation; hs.log2m = log2m; hs.rows = (int)rows;
  hs.registers.assign(host.begin() + (ptrdiff_t)first, host.begin() + (ptrdiff_t)(first + ((size_t)rows << log2m)));
  return hs;
}
// where hll_fold_kernel finds the long of a dictId: the device copy of the dictionary in the kernels' domain (ColumnDev)
static void fill_hll_dictionary(const ColumnDev& col, HllFoldParams* fp) {
  fp->dict32 = col.d_dict; fp->dict64 = col.d_dict64; fp->base = col.value_base;
  if (col.vkind == kValI32) fp->dict_kind = kHllDictI32;
  else if (col.vkind == kValI64) fp->dict_kind = kHllDictI64;
  else fp->dict_kind = col.stored_type == PG_TYPE_FLOAT ? kHllDictFloat : kHllDictDouble;
}
// ---- the set passes: what a pass query (kQueryDistinctPass / kQueryCountsPass) adds to the aggregation-only scan ----
// Five forms, each with kernels and a parameter block of its own, all keeping their device state in the context's d_distinct scratch (GROUP BY: one
// row per raw group id).  run_aggregation calls the stages below where a scalar query has nothing to do: bind (the columns and keys), arm (keys,
// layout, scratch, host buffers), launch, enqueue_post (what follows the kernel on the stream), harvest.
struct CollectLayout { size_t images[kMaxAggCols], work, heads, position, rows, rows_a, rows_b, temp, temp_bytes, total; };
constexpr size_t kCollectHeadBytes = 256;      // the scratch's first line: the cursor, the flag word, (later) a column's runs
struct SetPass {
  // Bitsets: DISTINCTCOUNT (and DISTINCTCOUNTHLL, folded behind the kernel) on dictionary columns; Counts: PERCENTILE on dictionary columns;
  // Collect: either function on raw columns; HllRaw: DISTINCTCOUNTHLL on raw columns; Moments: VARIANCE on raw and dictionary columns
  enum Form { None, Bitsets, Counts, Collect, HllRaw, Moments } form = None;
  int function = -1;                       // the one function besides COUNT(*) the pass query carries (set_pass_function)
  const char* name = "DISTINCTCOUNT";      // ... as the messages spell it
  std::vector<int> distinct_of;            // per aggregation: its bitset / counter row / list / register set (index into lw.distinct_slots), -1: none
  std::vector<int> hll_log2m_of;           // per aggregation: the log2m of a DISTINCTCOUNTHLL (0: another function)
  std::vector<int> key_cards;              // the key columns' cardinalities
  long long rows = 1;                      // raw group ids: their product
  DistinctParams dp; HllParams hp; CollectParams cp; MomentsParams mp;      // the form's parameter block (Bitsets and Counts: dp)
  std::vector<double> moments_host;        // Moments: where the {S1, S2} records (one per workgroup and column) or rows (GROUP BY: one per raw group id and column) land
  std::vector<std::vector<uint32_t>> distinct_host;      // Bitsets / Counts: per bitset where its copy lands -- the vector that becomes the result's DistinctSet, no second host copy
  // DISTINCTCOUNTHLL: per aggregation the first staged register word in the scratch (Bitsets: its own matrix's; HllRaw: its slot's); the staged
  // words are packed to bytes behind them and land in hll_host in the same order
  std::vector<size_t> hll_first;
  std::vector<int> hll_same_as;            // Bitsets: an earlier aggregation on the same column and log2m, whose registers this one shares
  size_t hll_staged_words = 0, hll_staged_first = 0;
  std::vector<uint8_t> hll_host;
  CollectLayout cl{};                                            // Collect: where everything lies in the scratch, ...
  unsigned long long collect_head[3] = {0ull, 0ull, 0ull};      // ... what the kernel leaves in its first line, and the lists' capacity in docs
  size_t collect_capacity = 0;
  // (declared last, destroyed first: nothing frees the host buffers above under a copy that is still on the stream)
  struct SyncOnExit { hipStream_t stream = nullptr; bool armed = false; ~SyncOnExit() { if (armed) (void)hipStreamSynchronize(stream); } } copy;
  bool grouped(const Lowered& lw) const { return !lw.distinct_key_slots.empty(); }
};
// bind, 1: which pass the query is.  (choose_scan_kernel and scan_grid go by the Lowered's flags and slots.)
static void open_set_pass(QueryRun& r, SetPass* p) {
  Lowered& lw = r.lw;
  const bool on = (r.q->flags & kQuerySetPass) != 0 && !r.want_bitmap;
  p->function = set_pass_function(r.q->flags);
  p->name = p->function == PG_AGG_PERCENTILE ? "PERCENTILE" : "DISTINCTCOUNT";
  lw.counts_pass = on && p->function == PG_AGG_PERCENTILE;
  lw.collect_pass = on && (r.q->flags & kQueryCollectPass) != 0;
  lw.hll_pass = on && (r.q->flags & kQueryHllPass) != 0;
  lw.moments_pass = on && (r.q->flags & kQueryMomentsPass) != 0;
  if (lw.moments_pass) p->name = "VARIANCE";
  if (!on) return;
  p->form = lw.moments_pass ? SetPass::Moments : lw.hll_pass ? SetPass::HllRaw : (lw.collect_pass ? SetPass::Collect : (lw.counts_pass ? SetPass::Counts : SetPass::Bitsets));
  p->copy.stream = r.ctx->stream;
  p->distinct_of.assign((size_t)std::max(r.na, 1), -1);
  p->hll_log2m_of.assign((size_t)std::max(r.na, 1), 0);
}
// bind, 2: aggregation `a`, if it is the pass's (*bound) -- its column's dictId stream (Bitsets / Counts) or value bytes (Collect / HllRaw).  One slot
// per distinct column (the same column twice shares it; a DISTINCTCOUNTHLL on a dictionary column shares the bitset too); HllRaw: per column and log2m.
static pg_status bind_set_pass_column(QueryRun& r, SetPass* p, int a, bool* bound) {
  const pg_segment* seg = r.seg; Lowered& lw = r.lw;
  const pg_aggregation& ag = r.q->aggregations[a];
  const bool hll_agg = p->function == PG_AGG_DISTINCTCOUNT && is_hll_function(ag.function);
  const bool moments_agg = lw.moments_pass && is_moments_function(ag.function);
  *bound = p->form != SetPass::None && (moments_agg || hll_agg || (ag.function == p->function && !lw.hll_pass && !lw.moments_pass));
  if (!*bound) return PG_OK;
  if (ag.column < 0 || ag.column >= (int)seg->cols.size()) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation column %d out of range", ag.column);
  if (hll_agg) p->hll_log2m_of[(size_t)a] = pg::hll_log2m_of(ag.function);
  const bool raw_form = lw.collect_pass || lw.hll_pass;
  // (the moments pass reads a column where it is stored, raw or dictionary-encoded: plan_moments checked it)
  if (!lw.moments_pass && seg->cols[(size_t)ag.column].encoding != (raw_form ? PG_FWD_RAW_FIXED_BYTE : PG_FWD_FIXED_BIT_DICT))
    return fail(PG_ERR_UNSUPPORTED, "%s on %s column %s", p->name, raw_form ? "dictionary" : "raw", seg->cols[(size_t)ag.column].name.c_str());
  r.add_projected(ag.column);
  const int s = slot_for(&lw, seg, ag.column, false);
  if (s < 0) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
  lw.plan.cols[s].in_agg = 1;
  size_t dc = 0;
  if (lw.hll_pass) { while (dc < lw.distinct_slots.size() && !(lw.distinct_slots[dc] == s && lw.hll_slot_log2m[dc] == p->hll_log2m_of[(size_t)a])) ++dc; }
  else dc = std::find(lw.distinct_slots.begin(), lw.distinct_slots.end(), s) - lw.distinct_slots.begin();
  if (dc == lw.distinct_slots.size()) {
    if (dc >= (size_t)kMaxAggCols) return fail(PG_ERR_UNSUPPORTED, "more than %d %s columns", kMaxAggCols, p->name);
    lw.distinct_slots.push_back(s);
    if (lw.hll_pass) lw.hll_slot_log2m.push_back(p->hll_log2m_of[(size_t)a]);
  }
  p->distinct_of[(size_t)a] = (int)dc;
  return PG_OK;
}
// bind, 3: the grouped kernels' keys -- dictionary columns, raw INT / LONG columns through their key images (built by the ordinary query before this pass)
static pg_status bind_set_pass_keys(QueryRun& r, SetPass* p) {
  pg_segment* seg = r.seg; const pg_query* q = r.q; Lowered& lw = r.lw;
  if (lw.distinct_slots.empty()) return fail(PG_ERR_INTERNAL, "a %s pass without a %s column", p->name, p->name);
  for (int g = 0; g < q->num_group_by; ++g) {
    int c = q->group_by_columns[g];
    if (c < 0 || c >= (int)seg->cols.size()) return fail(PG_ERR_INVALID_ARGUMENT, "group-by column %d out of range", c);
    r.add_projected(c);
    if (seg->cols[(size_t)c].encoding != PG_FWD_FIXED_BIT_DICT) { const pg_status st = ensure_key_image(seg, c, &c); if (st != PG_OK) return st; }
    if ((int)lw.distinct_key_slots.size() >= kMaxDistinctKeys) return fail(PG_ERR_UNSUPPORTED, "%s with more than %d group-by columns", p->name, kMaxDistinctKeys);
    const int s = slot_for(&lw, seg, c, false);
    if (s < 0) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
    lw.plan.cols[s].in_agg = 1;
    lw.distinct_key_slots.push_back(s);
    p->key_cards.push_back(std::max(seg->cols[(size_t)c].cardinality, 1));
  }
  return PG_OK;
}
// keys: the rows of every form's matrices -- one per raw group id -- and the kernels' mixed-radix decode of it
static pg_status set_pass_keys(const Lowered& lw, SetPass* p, DistinctParams* d) {
  for (int card : p->key_cards) p->rows *= card;
  if (p->rows > (long long)kMaxGroupSlots) return fail(PG_ERR_UNSUPPORTED, "%s GROUP BY over %lld raw keys", p->name, p->rows);
  d->num_cols = (int32_t)lw.distinct_slots.size();
  d->num_keys = (int32_t)lw.distinct_key_slots.size();
  uint32_t mult = 1;
  for (size_t g = 0; g < lw.distinct_key_slots.size(); ++g) {
    const DevColumn& kc = lw.plan.cols[lw.distinct_key_slots[g]];
    d->keys[g].fwd = kc.fwd; d->keys[g].bits = kc.bits; d->keys[g].mult = mult;
    mult *= (uint32_t)p->key_cards[g];
  }
  return PG_OK;
}
// arm, Bitsets / Counts: one zeroed bitset (counter vector) per column in the context's scratch -- under GROUP BY a matrix of one row per raw group
// id -- and behind the last row the slack of pg_set_pass_layout.h, so that a forward index that breaks the dictionary's bound cannot make the kernel
// write outside the allocation.  DISTINCTCOUNTHLLs on these columns: behind the bitsets one zeroed register matrix of 32-bit words per such
// aggregation (hll_fold_kernel's target), and behind those the same registers packed to bytes (hll_pack_kernel's) -- the only part of them that is copied.
static pg_status arm_bitsets(QueryRun& r, SetPass* p, const ScanGrid& grid) {
  ExecCtx* ctx = r.ctx; const Lowered& lw = r.lw; const int na = r.na;
  const bool counters = p->form == SetPass::Counts;
  DistinctParams& dp = p->dp;
  memset(&dp, 0, sizeof(dp));
  pg_status st = set_pass_keys(lw, p, &dp); if (st != PG_OK) return st;
  SetMatrixLayout matrices;
  size_t first[kMaxAggCols] = {};
  int lds_off = 0;
  for (size_t c = 0; c < lw.distinct_slots.size(); ++c) {
    const DevColumn& dc = lw.plan.cols[lw.distinct_slots[c]];
    DistinctCol& col = dp.cols[c];
    col.fwd = dc.fwd; col.bits = dc.bits; col.words = set_row_words(counters, dc.cardinality); col.lds_off = lds_off;
    lds_off += col.words;
    first[c] = (size_t)matrices.add(counters, (uint64_t)p->rows, dc.bits, dc.cardinality);
  }
  dp.lds_words = grid.distinct_lds ? lds_off : 0;
  p->hll_first.assign((size_t)std::max(na, 1), 0);
  p->hll_same_as.assign((size_t)std::max(na, 1), -1);
  size_t hll_words = 0;
  const size_t hll_base = (size_t)hll_staged_base(matrices.total_words());
  for (int a = 0; a < na; ++a) {
    if (p->hll_log2m_of[(size_t)a] == 0) continue;
    // (the same column at the same log2m twice: one register matrix, one fold)
    for (int b = 0; b < a && p->hll_same_as[(size_t)a] < 0; ++b)
      if (p->hll_log2m_of[(size_t)b] == p->hll_log2m_of[(size_t)a] && p->distinct_of[(size_t)b] == p->distinct_of[(size_t)a]) p->hll_same_as[(size_t)a] = b;
    if (p->hll_same_as[(size_t)a] >= 0) { p->hll_first[(size_t)a] = p->hll_first[(size_t)p->hll_same_as[(size_t)a]]; continue; }
    p->hll_first[(size_t)a] = hll_base + hll_words;
    hll_words += (size_t)hll_staged_words((uint64_t)p->rows, p->hll_log2m_of[(size_t)a]);
  }
  st = ensure_distinct(r.seg, ctx, (size_t)hll_scratch_words(hll_base, hll_words)); if (st != PG_OK) return st;
  for (size_t c = 0; c < lw.distinct_slots.size(); ++c) dp.cols[c].set_bits = ctx->d_distinct + first[c];
  HIP_TRY(hipMemsetAsync(ctx->d_distinct, 0, (hll_base + hll_words) * 4, ctx->stream));
  p->hll_staged_words = hll_words; p->hll_staged_first = hll_base;
  if (r.out) {
    p->distinct_host.resize(lw.distinct_slots.size());
    // (a bitset that only HLLs use stays on the device)
    for (int a = 0; a < na; ++a) {
      const int dc = p->distinct_of[(size_t)a];
      if (dc >= 0 && p->hll_log2m_of[(size_t)a] == 0) p->distinct_host[(size_t)dc].resize((size_t)p->rows * (size_t)dp.cols[dc].words);
    }
    p->hll_host.resize(hll_words);
  }
  return PG_OK;
}
// arm, HllRaw: one zeroed register row per slot in the same scratch -- under GROUP BY a matrix of one row per raw group id -- and the packed bytes behind them
static pg_status arm_hll_raw(QueryRun& r, SetPass* p) {
  ExecCtx* ctx = r.ctx; const Lowered& lw = r.lw;
  HllParams& hp = p->hp;
  memset(&hp, 0, sizeof(hp));
  pg_status st = set_pass_keys(lw, p, &hp.d); if (st != PG_OK) return st;
  size_t hll_words = 0, slot_first[kMaxAggCols] = {};
  int lds_off = 0;
  for (size_t c = 0; c < lw.distinct_slots.size(); ++c) {
    const DevColumn& dc = lw.plan.cols[lw.distinct_slots[c]];
    hp.fwd[c] = dc.fwd; hp.wide[c] = (dc.vkind == kValI64 || dc.vkind == kValF64) ? 1 : 0;
    hp.log2m[c] = lw.hll_slot_log2m[c]; hp.lds_off[c] = lds_off;
    lds_off += 1 << hp.log2m[c];
    slot_first[c] = hll_words;
    hll_words += (size_t)hll_staged_words((uint64_t)p->rows, hp.log2m[c]);
  }
  hp.lds_words = p->grouped(lw) ? 0 : lds_off;      // (scan_hll_kernel keeps the registers in LDS; group_hll_kernel's matrices live in HBM)
  hp.num_rows = (uint32_t)p->rows;
  st = ensure_distinct(r.seg, ctx, (size_t)hll_scratch_words(0, hll_words)); if (st != PG_OK) return st;
  for (size_t c = 0; c < lw.distinct_slots.size(); ++c) hp.regs[c] = ctx->d_distinct + slot_first[c];
  p->hll_first.assign((size_t)std::max(r.na, 1), 0);
  for (int a = 0; a < r.na; ++a) if (p->distinct_of[(size_t)a] >= 0) p->hll_first[(size_t)a] = slot_first[p->distinct_of[(size_t)a]];
  HIP_TRY(hipMemsetAsync(ctx->d_distinct, 0, hll_words * 4, ctx->stream));
  p->hll_staged_words = hll_words; p->hll_staged_first = 0;
  if (r.out) p->hll_host.resize(hll_words);
  return PG_OK;
}
// arm, Collect: one list of `capacity` 64-bit images per raw column in the same scratch (GROUP BY: the docs' raw group ids beside them), the sort's
// second buffers, the run arrays and rocPRIM's scratch behind them.  The capacity is the segment's docs -- what the plan-time bound was priced
// with (plan_collect_bytes) -- so no reservation of a matching doc can fail; the kernel checks every one all the same.
static pg_status arm_collect(QueryRun& r, SetPass* p) {
  ExecCtx* ctx = r.ctx; const Lowered& lw = r.lw;
  CollectParams& cp = p->cp; CollectLayout& cl = p->cl;
  memset(&cp, 0, sizeof(cp));
  pg_status st = set_pass_keys(lw, p, &cp.d); if (st != PG_OK) return st;
  const bool grouped = p->grouped(lw);
  const size_t capacity = p->collect_capacity = (size_t)std::max<long long>((long long)r.seg->num_docs, 1);
  HIP_TRY(collect_sort_temp_bytes(capacity, grouped, &cl.temp_bytes));
  auto take = [&cl](size_t bytes) { const size_t at = cl.total; cl.total += (bytes + 255) & ~(size_t)255; return at; };
  (void)take(kCollectHeadBytes);
  for (size_t c = 0; c < lw.distinct_slots.size(); ++c) cl.images[c] = take(capacity * 8);
  cl.work = take(capacity * 8);
  cl.heads = take(capacity * 4);
  cl.position = take(capacity * 4);
  if (grouped) { cl.rows = take(capacity * 4); cl.rows_a = take(capacity * 4); cl.rows_b = take(capacity * 4); }
  cl.temp = take(std::max<size_t>(cl.temp_bytes, 256));
  st = ensure_distinct(r.seg, ctx, cl.total / 4); if (st != PG_OK) return st;
  uint8_t* const base = reinterpret_cast<uint8_t*>(ctx->d_distinct);
  for (size_t c = 0; c < lw.distinct_slots.size(); ++c) {
    const DevColumn& dc = lw.plan.cols[lw.distinct_slots[c]];
    cp.fwd[c] = dc.fwd; cp.vkind[c] = dc.vkind;
    cp.out_images[c] = reinterpret_cast<unsigned long long*>(base + cl.images[c]);
  }
  cp.out_rows = grouped ? reinterpret_cast<uint32_t*>(base + cl.rows) : nullptr;
  cp.cursor = reinterpret_cast<unsigned long long*>(base);
  cp.flags = reinterpret_cast<uint32_t*>(base + 8);
  cp.capacity = (unsigned long long)capacity;
  HIP_TRY(hipMemsetAsync(base, 0, kCollectHeadBytes, ctx->stream));
  return PG_OK;
}
// arm, Moments: the kernels' value sources, the pivots execute_moments took from the ordinary query, and the scratch -- without GROUP BY one
// {S1, S2} record per workgroup and column, which every workgroup writes; under GROUP BY a zeroed [rows x cols] matrix of {S1, S2} and behind it the
// uploaded [rows x cols] pivots.
static thread_local const std::vector<double>* t_moments_pivots = nullptr;      // execute_moments -> arm_moments, around the pass's execute_one
static pg_status arm_moments(QueryRun& r, SetPass* p, const ScanGrid& grid) {
  ExecCtx* ctx = r.ctx; const Lowered& lw = r.lw; const pg_segment* seg = r.seg;
  MomentsParams& mp = p->mp;
  memset(&mp, 0, sizeof(mp));
  pg_status st = set_pass_keys(lw, p, &mp.d); if (st != PG_OK) return st;
  const size_t cols = lw.distinct_slots.size();
  for (int a = 0; a < r.na; ++a) {
    const int c = p->distinct_of[(size_t)a];
    if (c < 0) continue;
    const ColumnDev& col = seg->cols[(size_t)r.q->aggregations[a].column];
    const DevColumn& dc = lw.plan.cols[lw.distinct_slots[(size_t)c]];
    MomentsCol& mc = mp.cols[c];
    mc.fwd = dc.fwd; mc.bits = dc.bits; mc.cardinality = col.cardinality;
    if (col.encoding == PG_FWD_FIXED_BIT_DICT) {
      mc.dict32 = col.d_dict; mc.dict64 = col.d_dict64; mc.base = col.value_base;
      mc.source = col.vkind == kValI32 ? kMomentsDictI32 : (col.vkind == kValI64 ? kMomentsDictI64 : kMomentsDictF64);
      if ((mc.source == kMomentsDictI32 ? (const void*)mc.dict32 : (const void*)mc.dict64) == nullptr || col.cardinality < 1)
        return fail(PG_ERR_INTERNAL, "VARIANCE on column %s: no device copy of its dictionary", col.name.c_str());
    } else {
      mc.source = col.stored_type == PG_TYPE_INT ? kMomentsRawI32 : (col.stored_type == PG_TYPE_LONG ? kMomentsRawI64 : (col.stored_type == PG_TYPE_FLOAT ? kMomentsRawF32 : kMomentsRawF64));
    }
    if (mc.fwd == nullptr) return fail(PG_ERR_INTERNAL, "VARIANCE on column %s: no forward index on the device", col.name.c_str());
  }
  const bool grouped = p->grouped(lw);
  const std::vector<double>* pivots = t_moments_pivots;
  if (pivots == nullptr || pivots->size() != (size_t)p->rows * cols) return fail(PG_ERR_INTERNAL, "the VARIANCE pass without the pivots of %lld rows x %zu columns", p->rows, cols);
  const size_t out_doubles = (grouped ? (size_t)p->rows : (size_t)grid.blocks) * cols * 2, pivot_doubles = grouped ? pivots->size() : 0;
  st = ensure_distinct(r.seg, ctx, (out_doubles + pivot_doubles) * 2); if (st != PG_OK) return st;
  double* const base = reinterpret_cast<double*>(ctx->d_distinct);
  mp.out = base;
  if (grouped) {
    mp.pivots = base + out_doubles;
    mp.num_rows = (uint32_t)p->rows;
    HIP_TRY(hipMemsetAsync(base, 0, out_doubles * 8, ctx->stream));
    HIP_TRY(hipMemcpyAsync(base + out_doubles, pivots->data(), pivot_doubles * 8, hipMemcpyHostToDevice, ctx->stream));
  } else {
    for (size_t c = 0; c < cols; ++c) mp.pivot[c] = (*pivots)[c];
  }
  if (r.out) p->moments_host.resize(out_doubles);
  return PG_OK;
}
static pg_status arm_set_pass(QueryRun& r, SetPass* p, const ScanGrid& grid) {
  switch (p->form) {
    case SetPass::Moments: return arm_moments(r, p, grid);
    case SetPass::Bitsets: case SetPass::Counts: return arm_bitsets(r, p, grid);
    case SetPass::Collect: return arm_collect(r, p);
    case SetPass::HllRaw: return arm_hll_raw(r, p);
    default: return PG_OK;
  }
}
// launch: the form's kernel behind the lowered filter -- the scan form without GROUP BY, the group form with it
static void launch_set_pass(const QueryRun& r, SetPass* p, const ScanGrid& grid) {
  const ScanParams& sp = r.lw.sp; hipStream_t stream = r.ctx->stream;
  const bool grouped = p->grouped(r.lw); const int blocks = grid.blocks; const size_t lds = grid.lds;
  switch (p->form) {
    case SetPass::Bitsets: p->dp.scan = sp; grouped ? launch_group_distinct(blocks, lds, stream, p->dp) : launch_scan_distinct(grid.distinct_lds, blocks, lds, stream, p->dp); break;
    case SetPass::Counts: p->dp.scan = sp; grouped ? launch_group_counts(blocks, lds, stream, p->dp) : launch_scan_counts(grid.distinct_lds, blocks, lds, stream, p->dp); break;
    case SetPass::Collect: p->cp.d.scan = sp; grouped ? launch_group_collect(blocks, lds, stream, p->cp) : launch_scan_collect(blocks, lds, stream, p->cp); break;
    case SetPass::HllRaw: p->hp.d.scan = sp; grouped ? launch_group_hll(blocks, lds, stream, p->hp) : launch_scan_hll(blocks, lds, stream, p->hp); break;
    case SetPass::Moments: p->mp.d.scan = sp; grouped ? launch_group_moments(blocks, lds, stream, p->mp) : launch_scan_moments(blocks, lds, stream, p->mp); break;
    default: break;
  }
}
// enqueue_post: what follows the kernel on the stream -- the bitsets' / counters' copies; the collect pass's cursor and flag word; one hll_fold_kernel
// per DISTINCTCOUNTHLL aggregation over its column's bitset rows, then hll_pack_kernel over all staged registers and the copy of the packed bytes
static pg_status enqueue_set_pass_post(QueryRun& r, SetPass* p) {
  const pg_segment* seg = r.seg; ExecCtx* ctx = r.ctx;
  const bool bitsets = p->form == SetPass::Bitsets || p->form == SetPass::Counts;
  if (bitsets && !p->distinct_host.empty()) {
    p->copy.armed = true;
    for (size_t c = 0; c < p->distinct_host.size(); ++c)
      if (!p->distinct_host[c].empty()) HIP_TRY(hipMemcpyAsync(p->distinct_host[c].data(), p->dp.cols[c].set_bits, p->distinct_host[c].size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (p->form == SetPass::Collect) { p->copy.armed = true; HIP_TRY(hipMemcpyAsync(p->collect_head, ctx->d_distinct, 16, hipMemcpyDeviceToHost, ctx->stream)); }
  if (p->form == SetPass::Moments && !p->moments_host.empty()) {
    p->copy.armed = true;
    HIP_TRY(hipMemcpyAsync(p->moments_host.data(), p->mp.out, p->moments_host.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (p->hll_staged_words == 0) return PG_OK;
  for (int a = 0; a < (bitsets ? r.na : 0); ++a) {      // the bitsets' rows -> register rows, one fold per DISTINCTCOUNTHLL aggregation over its column's bitset
    if (p->hll_log2m_of[(size_t)a] == 0 || p->hll_same_as[(size_t)a] >= 0) continue;
    const ColumnDev& col = seg->cols[(size_t)r.q->aggregations[a].column];
    const DistinctCol& bits = p->dp.cols[p->distinct_of[(size_t)a]];
    HllFoldParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.bits = bits.set_bits; fp.regs = ctx->d_distinct + p->hll_first[(size_t)a];
    fp.words = bits.words; fp.cardinality = col.cardinality; fp.log2m = p->hll_log2m_of[(size_t)a];
    fill_hll_dictionary(col, &fp);
    launch_hll_fold(p->rows, ctx->stream, fp);
    HIP_TRY(hipGetLastError());
  }
  uint8_t* const packed = reinterpret_cast<uint8_t*>(ctx->d_distinct + p->hll_staged_first + p->hll_staged_words);
  launch_hll_pack(ctx->d_distinct + p->hll_staged_first, packed, p->hll_staged_words, seg->num_cus, ctx->stream);
  HIP_TRY(hipGetLastError());
  if (!p->hll_host.empty()) { p->copy.armed = true; HIP_TRY(hipMemcpyAsync(p->hll_host.data(), packed, p->hll_host.size(), hipMemcpyDeviceToHost, ctx->stream)); }
  return PG_OK;
}
// harvest, Bitsets / Counts / HllRaw: one set per DISTINCTCOUNT / PERCENTILE aggregation, one register set per DISTINCTCOUNTHLL.  Aggregation only: a
// DISTINCTCOUNT's count is its set's cardinality, an HLL's its non-zero registers.  Under GROUP BY the rows are raw group ids: execute_distinct /
// execute_percentile keep the rows of the groups that exist.
static void harvest_sets(QueryRun& r, SetPass* p) {
  pg_result* out = r.out; const bool grouped = p->grouped(r.lw);
  std::unique_ptr<ResultInternal> sets(new ResultInternal());
  for (int a = r.na - 1; a >= 0; --a) {      // (the last aggregation on a column takes the copy itself, earlier ones on the same column a copy of it)
    const int dc = p->distinct_of[(size_t)a];
    if (dc < 0) continue;
    if (p->hll_log2m_of[(size_t)a] != 0) {
      sets->hll.push_back(hll_set_of(p->hll_host, p->hll_first[(size_t)a] - p->hll_staged_first, a, p->hll_log2m_of[(size_t)a], p->rows));
      if (!grouped) out->aggregations[a].count = hll_nonzero(sets->hll.back().registers.data(), sets->hll.back().registers.size());
      continue;
    }
    DistinctSet ds;
    ds.aggregation = a; ds.num_words = p->dp.cols[dc].words; ds.rows = (int)p->rows;
    bool again = false;
    for (int b = 0; b < a; ++b) again |= p->distinct_of[(size_t)b] == dc && p->hll_log2m_of[(size_t)b] == 0;
    if (again) ds.words = p->distinct_host[(size_t)dc]; else ds.words = std::move(p->distinct_host[(size_t)dc]);
    if (!grouped && p->form == SetPass::Bitsets) {      // (PERCENTILE: count stays the docs aggregated, the list's length)
      int64_t card = 0;
      for (uint32_t w : ds.words) card += __builtin_popcount(w);
      out->aggregations[a].count = card;
    }
    sets->distinct.push_back(std::move(ds));
  }
  out->internal = sets.release();
}
// harvest, Collect: the cursor's final value is the filter's match count (`matched`: the scan record's).  Every column's list is sorted and
// run-length encoded on the device; only the runs cross the bus.
static pg_status harvest_collect(QueryRun& r, SetPass* p, unsigned long long matched) {
  pg_segment* seg = r.seg; ExecCtx* ctx = r.ctx; const Lowered& lw = r.lw; pg_result* out = r.out;
  const CollectLayout& cl = p->cl;
  struct Trim { pg_segment* seg; ExecCtx* ctx; ~Trim() { trim_distinct(seg, ctx); } } trim_on_exit{seg, ctx};
  const unsigned long long n = p->collect_head[0];
  if ((uint32_t)p->collect_head[1] & kCollectOverflow) return fail(PG_ERR_INTERNAL, "%s: the value lists overflowed their capacity of %zu docs (cursor %llu)", p->name, p->collect_capacity, n);
  if (n != matched) return fail(PG_ERR_INTERNAL, "%s: %llu values were collected for %llu matching docs", p->name, n, matched);
  if (!out) return PG_OK;
  const bool grouped = p->grouped(lw);
  uint8_t* const base = reinterpret_cast<uint8_t*>(ctx->d_distinct);
  int row_bits = 1;
  while (row_bits < 32 && (1ll << row_bits) < p->rows) ++row_bits;
  std::vector<ValueList> per_col(lw.distinct_slots.size());
  std::vector<uint32_t> first;
  for (size_t c = 0; c < lw.distinct_slots.size(); ++c) {
    ValueList& vl = per_col[c];
    vl.grouped_in_transit = grouped;
    if (n == 0) continue;
    CollectSort cs;
    cs.images = p->cp.out_images[c]; cs.images_work = reinterpret_cast<unsigned long long*>(base + cl.work);
    cs.rows = p->cp.out_rows; cs.rows_a = reinterpret_cast<uint32_t*>(base + cl.rows_a); cs.rows_b = reinterpret_cast<uint32_t*>(base + cl.rows_b);
    cs.row_bits = row_bits;
    cs.heads = reinterpret_cast<uint32_t*>(base + cl.heads); cs.position = reinterpret_cast<uint32_t*>(base + cl.position);
    cs.num_runs = reinterpret_cast<uint32_t*>(base + 16);
    cs.temp = base + cl.temp; cs.temp_bytes = std::max<size_t>(cl.temp_bytes, 256);
    CollectRuns runs;
    HIP_TRY(collect_sort_runs(cs, (size_t)n, seg->num_cus, ctx->stream, &runs));
    uint32_t num_runs = 0;
    HIP_TRY(hipMemcpyAsync(&num_runs, cs.num_runs, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (num_runs == 0u || (unsigned long long)num_runs > n) return fail(PG_ERR_INTERNAL, "%s: %u runs in a list of %llu values", p->name, num_runs, n);
    // only the runs cross the bus: their images, the index of their first entry and (GROUP BY) their raw group ids
    vl.value_bits.resize(num_runs); first.resize(num_runs);
    HIP_TRY(hipMemcpyAsync(vl.value_bits.data(), runs.images, (size_t)num_runs * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(first.data(), runs.first, (size_t)num_runs * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (grouped) { vl.run_rows.resize(num_runs); HIP_TRY(hipMemcpyAsync(vl.run_rows.data(), runs.rows, (size_t)num_runs * 4, hipMemcpyDeviceToHost, ctx->stream)); }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const bool floating = p->cp.vkind[c] == kValF64 || p->cp.vkind[c] == kValF32;
    vl.counts.resize(num_runs);
    for (uint32_t j = 0; j < num_runs; ++j) {
      vl.value_bits[j] = (int64_t)rank_image_value_bits((unsigned long long)vl.value_bits[j], floating);
      vl.counts[j] = (j + 1 < num_runs ? first[j + 1] : (uint32_t)n) - first[j];
    }
  }
  std::unique_ptr<ResultInternal> lists(new ResultInternal());
  for (int a = r.na - 1; a >= 0; --a) {      // (the last aggregation on a column takes the runs themselves, earlier ones on the same column a copy)
    const int dc = p->distinct_of[(size_t)a];
    if (dc < 0) continue;
    bool again = false;
    for (int b = 0; b < a; ++b) again |= p->distinct_of[(size_t)b] == dc;
    ValueList vl;
    if (again) vl = per_col[(size_t)dc]; else vl = std::move(per_col[(size_t)dc]);
    vl.aggregation = a;
    vl.offsets = {0, vl.value_bits.size()};
    // aggregation only: PERCENTILE's count is the list's length (the docs aggregated: convert put it there), DISTINCTCOUNT's the number of runs
    if (!grouped && p->function == PG_AGG_DISTINCTCOUNT) out->aggregations[a].count = (int64_t)vl.value_bits.size();
    lists->values.push_back(std::move(vl));
  }
  out->internal = lists.release();
  return PG_OK;
}
// harvest, Moments: {S1, S2} per VARIANCE aggregation -- without GROUP BY the workgroups' records added in workgroup order (the same grid adds
// the same numbers in the same order: bit-identical run to run), under GROUP BY the rows of all raw group ids.  execute_moments turns them into m2.
static void harvest_moments(QueryRun& r, SetPass* p) {
  const size_t cols = r.lw.distinct_slots.size();
  const bool grouped = p->grouped(r.lw);
  const size_t records = p->moments_host.size() / (cols * 2);      // workgroups, or raw group ids
  std::unique_ptr<ResultInternal> sets(new ResultInternal());
  for (int a = 0; a < r.na; ++a) {
    const int dc = p->distinct_of[(size_t)a];
    if (dc < 0) continue;
    MomentsSet ms;
    ms.aggregation = a; ms.rows = grouped ? (int)records : 1;
    if (grouped) {
      ms.m2.resize(records * 2);
      for (size_t row = 0; row < records; ++row) { ms.m2[2 * row] = p->moments_host[(row * cols + (size_t)dc) * 2]; ms.m2[2 * row + 1] = p->moments_host[(row * cols + (size_t)dc) * 2 + 1]; }
    } else {
      double s1 = 0.0, s2 = 0.0;
      for (size_t b = 0; b < records; ++b) { s1 += p->moments_host[(b * cols + (size_t)dc) * 2]; s2 += p->moments_host[(b * cols + (size_t)dc) * 2 + 1]; }
      ms.m2 = {s1, s2};
    }
    sets->moments.push_back(std::move(ms));
  }
  r.out->internal = sets.release();
}
// harvest: the stream was synchronised -- the copies of enqueue_post have landed.  The sets go to out->internal for execute_distinct / execute_percentile.
static pg_status harvest_set_pass(QueryRun& r, SetPass* p, const BlockPartial& fp) {
  p->copy.armed = false;
  if (p->form == SetPass::Collect) return harvest_collect(r, p, (unsigned long long)fp.count);
  if (r.out) { if (p->form == SetPass::Moments) harvest_moments(r, p); else harvest_sets(r, p); }
  trim_distinct(r.seg, r.ctx);
  return PG_OK;
}
// ---------------- aggregation only ----------------
static pg_status run_aggregation(QueryRun& r, unsigned long long* d_out_bitmap_request, uint64_t* host_bitmap, int64_t host_bitmap_words, int64_t* out_cardinality) {
  pg_segment* seg = r.seg; const pg_query* q = r.q; pg_result* out = r.out; ExecCtx* ctx = r.ctx; Lowered& lw = r.lw; ScanParams& sp = lw.sp;
  PlanParams& pl = lw.plan; const int na = r.na, num_cols_total = (int)seg->cols.size(); const bool want_bitmap = r.want_bitmap, timed = r.timed;
  pg_status st = PG_OK;
  std::vector<int> agg_slot_of((size_t)std::max(na, 1), -1);
  SetPass pass;      // (form None: an ordinary query -- every stage below is skipped)
  open_set_pass(r, &pass);
  for (int a = 0; a < na; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    if (ag.function == PG_AGG_COUNT) {
      if ((q->flags & kQueryCountReadsColumn) && ag.column >= 0 && ag.column < num_cols_total) r.add_projected(ag.column);
      continue;
    }
    bool bound = false;
    st = bind_set_pass_column(r, &pass, a, &bound); if (st != PG_OK) return st;
    if (bound) continue;
    if (ag.function < PG_AGG_COUNT || ag.function > PG_AGG_AVG || pass.form != SetPass::None) return fail(PG_ERR_UNSUPPORTED, "aggregation function %d", ag.function);
    if (ag.column < 0 || ag.column >= num_cols_total) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation column %d out of range", ag.column);
    r.add_projected(ag.column);
    int s = slot_for(&lw, seg, ag.column, lw.plane_cols[(size_t)ag.column] != 0);
    if (s < 0) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
    pl.cols[s].in_agg = 1;
    int ac = -1;
    for (int i = 0; i < pl.num_agg_cols; ++i) if (pl.agg_cols[i].col == s) ac = i;
    if (ac < 0) {
      if (pl.num_agg_cols >= kMaxAggCols) return fail(PG_ERR_UNSUPPORTED, "more than %d aggregated columns", kMaxAggCols);
      ac = pl.num_agg_cols++;
      pl.agg_cols[ac] = PlanAggCol{s, 0, 0, 0};
    }
    if (ag.function == PG_AGG_SUM || ag.function == PG_AGG_AVG) pl.agg_cols[ac].need_sum = 1;
    if (ag.function == PG_AGG_MIN || ag.function == PG_AGG_MAX) pl.agg_cols[ac].need_minmax = 1;
    agg_slot_of[(size_t)a] = ac;
  }
  if (pass.form != SetPass::None) { st = bind_set_pass_keys(r, &pass); if (st != PG_OK) return st; }
  bool need_queue = false, typed = false;
  for (int i = 0; i < pl.num_agg_cols; ++i) {
    const DevColumn& c = pl.cols[pl.agg_cols[i].col];
    need_queue |= pl.agg_cols[i].need_sum && !c.is_raw && !c.is_plane && c.vkind == kValI32;
    typed |= c.vkind != kValI32 && (pl.agg_cols[i].need_sum || c.is_raw);     // 8-byte / floating-point values are read
  }
  Geometry geo;
  finish_geometry(seg, &lw, 0, need_queue, kBlockThreads / 64, waves_scan_agg(pl.num_agg_cols <= 1, typed), &geo);
  ScanChoice k = choose_scan_kernel(seg, lw, r.hist_col, typed, want_bitmap, out != nullptr);
  if (k.kernel == ScanKernel::Agg && (size_t)sp.wave_lds_bytes > kLdsBudget) return fail(PG_ERR_UNSUPPORTED, "query needs %d bytes of LDS per wavefront", sp.wave_lds_bytes);
  if (k.kernel == ScanKernel::SimpleValid) {
    // scan_simple_valid_kernel's parameter block: the doc set's words in bitmaps[0], the range leaf (if any) as the one node.  Every doc of
    // the set is looked at once by the scan leaf behind it (ScanBasedDocIdIterator.applyAnd over the bitmap's docs): the entry count is the
    // set's cardinality, known since pg_doc_set_create -- the kernel carries no counter.
    sp.bitmaps[0] = pl.leaves[lw.valid_leaf].bitmap;
    if (sp.num_nodes == 3) { sp.nodes[0] = sp.nodes[1]; sp.nodes[0].flags = 0; sp.num_nodes = 1; }
    else sp.num_nodes = 0;
    int64_t card = 0;
    for (const auto& ds : lw.doc_sets) if (ds->d_words == pl.leaves[lw.valid_leaf].bitmap) card = ds->cardinality;
    lw.stats_closed_entries = sp.num_nodes == 1 ? card : 0;
    lw.stats_chain_flagged = false;
  }
  const ScanGrid grid = scan_grid(seg, k, lw, geo, pl.num_agg_cols, r.hist_col);
  const int blocks = grid.blocks;
  if (k.kernel == ScanKernel::Hist) { sp.hist_slot = k.hist_slot; sp.hist_bins = seg->cols[(size_t)r.hist_col].cardinality; }
  sp.speculate = 1;
  sp.profile = (g_engine.flags & PG_CFG_PROFILE_WAVES) ? 1 : 0;
  st = ensure_partials(ctx, blocks); if (st != PG_OK) return st;
  sp.partials = ctx->d_partials;
  sp.out_bitmap = nullptr;
  if (want_bitmap) {
    st = ensure_bitmap(seg, ctx, 0); if (st != PG_OK) return st;
    sp.out_bitmap = ctx->d_bitmaps[0];
  }
  sp.sparse_windows = nullptr; sp.sparse_num_windows = 0;
  bool defer_index_and = false;
  const unsigned long long seq = ++ctx->seq;      // the sequence number the query's folded record is published under (a gathering index_and_kernel's, or the scan kernel's)
  const bool lane_private = k.general != ScanKernel::Agg;      // a lane-private kernel, or one specialised from it
  if (k.kernel == ScanKernel::Sparse) {
    // A handful of survivors per window (the planner's estimate from the postings' sizes: independent predicates): index_and_kernel reads
    // their values itself -- ONE launch for `SUM(v) WHERE p = 3 AND q = 5 AND r = 7` (BASELINE.json configs[4]); else scan_sparse_kernel
    // walks the window masks behind it (no list, no index_and_finalize_kernel between the two kernels).  PINOT_GPU_INDEX_GATHER=0: never.
    const bool gather = g_engine.index_gather && lw.and_pending && lw.index_and_is_whole_filter && out && pl.num_agg_cols <= kMaxAndGather &&
                        lw.and_expected_docs <= 4.0 * (double)lw.finalize_windows;
    defer_index_and = gather && r.defer != nullptr && !r.defer->single && g_engine.batch_index && g_engine.direct_result && !want_bitmap && index_and_shares_a_launch(lw);
    if (defer_index_and) arm_index_gather(&lw, &sp);      // (launched by the batch: BatchKind::IndexAnd)
    else st = launch_index_and(&lw, ctx, gather ? &sp : nullptr);
    if (st != PG_OK) return st;
    sp.tile_list = lw.tile_list; sp.tile_count = lw.tile_count;      // (not read by the kernel; "listed" is what the planner and the statistics go by)
    sp.sparse_windows = lw.and_info; sp.sparse_num_windows = (int32_t)lw.finalize_windows;
  } else if (!want_bitmap && lane_private) {
    st = complete_index_list(&lw, ctx); if (st != PG_OK) return st;
    sp.tile_list = lw.tile_list; sp.tile_count = lw.tile_count;
  }
  else { st = complete_index_and_bitmap(&lw, ctx); if (st != PG_OK) return st; }
  const bool count_leap2 = out && lw.stats_leap2_flagged && k.kernel != ScanKernel::Narrow && k.kernel != ScanKernel::NarrowSingle && lane_private;
  const bool count_entries = (out && lw.stats_chain_flagged && lane_private) || count_leap2;
  if (lw.side != nullptr) {
    // the transducer pass behind this query: a kernel that evaluates the filter with eval_filter_private over every tile leaves the leaves' bitmaps behind
    const bool wrote = kScanKernels[(int)k.kernel].writes_leaves && sp.tile_list == nullptr;
    for (int l = 0; l < kMaxLeaves; ++l) sp.leaf_out[l] = wrote ? lw.sp_leaf_out[l] : nullptr;
    sp.leaf_out_enabled = wrote ? 1 : 0;
    lw.side->kernel_wrote = wrote;
  }
  // The transducer walked INSIDE the general lane-private kernel (scan_private_fsm_kernel): machines of at most four states over at most
  // four inputs, every input a leaf of its own in the lowered filter.  No leaf bitmap is written or read back; the tiles' tables are
  // joined by fsm_chain_kernel / fsm_finish_kernel behind the scan, on the query's stream.  PINOT_GPU_FSM_FUSED=0: the separate pass.
  sp.fsm_tables = nullptr; sp.fsm_states = 0; sp.fsm_inputs = 0;
  // (NOT in scan_narrow_kernel: measured on `COUNT(*) WHERE p = 3 AND q = 5 AND r = 7` over 4 / 6 / 8-bit columns, 1 B rows -- the walk takes the
  //  kernel from 164 to 199 registers, three to two waves per SIMD, 0.53 -> 0.85 ms, more than the 0.24 ms pass it replaces: 0.767 -> 0.868 ms
  //  for the query; the same query through this kernel: 1.06 ms.  profiles/r5/fsm_walk_inside_the_scan_ab.txt)
  if (lw.side != nullptr && sp.leaf_out_enabled != 0 && g_engine.fsm_fused && g_engine.fsm_perm && k.kernel == ScanKernel::Private && out) {
    const fstats::Fsm& f = *lw.side->fsm;
    int max_inc = 0;
    for (uint8_t d : f.delta) max_inc = std::max(max_inc, (int)(d >> 4));
    bool fits = f.num_states <= 4 && f.num_inputs <= 4 && max_inc <= 7 && !f.has_episodes();      // (episodes need the second walk of the pass)
    for (int i = 0; i < f.num_inputs && fits; ++i) fits = lw.side->mapped[i];
    if (fits) {
      k.kernel = ScanKernel::PrivateFsm;
      sp.fsm_tables = lw.side->tables; sp.fsm_states = f.num_states; sp.fsm_inputs = f.num_inputs;
      for (int l = 0; l < kMaxLeaves; ++l) {
        sp.fsm_input_of_leaf[l] = -1;
        for (int i = 0; i < f.num_inputs; ++i) if (sp.leaf_out[l] != nullptr && sp.leaf_out[l] == lw.side->bitmap[i]) sp.fsm_input_of_leaf[l] = (int8_t)i;
        sp.leaf_out[l] = nullptr;
      }
      sp.leaf_out_enabled = 0;
      memset(sp.fsm_delta, 0, sizeof(sp.fsm_delta));
      for (int st8 = 0; st8 < f.num_states; ++st8)
        for (int in = 0; in < (1 << f.num_inputs); ++in) sp.fsm_delta[(st8 << 4) | in] = f.delta[(size_t)((st8 << f.num_inputs) | in)];
      if (!ctx->h_filter_entries) HIP_TRY(hipHostMalloc((void**)&ctx->h_filter_entries, 8, hipHostMallocDefault));
    }
  }
  sp.filter_entries = nullptr;
  sp.leap_tables = nullptr;
  if (count_leap2) { st = arm_leap_tables(seg, ctx, &sp.leap_tables, nullptr); if (st != PG_OK) return st; }
  else if (lw.stats_leap2_flagged) for (int n = 0; n < sp.num_nodes; ++n) sp.nodes[n].flags &= ~kNodeLeapfrog2;      // a kernel without the count runs this query
  sp.raw64_coalesced = g_engine.raw64_coalesced ? 1 : 0;
  // (the entries counted by the kernel travel in its record: BlockPartial.entries -- no counter to zero, no copy command)
  // The folded record -> the reference's holder types.  Everything is captured by value: pg_execute_batch calls it after this function
  // has returned (the query, the segment and the context's pinned counter outlive the batch).
  const int kernel_id = lw.gathered ? PG_KERNEL_INDEX_AND : kScanKernels[(int)k.kernel].id;
  const HostRecord* host_record = ctx->h_record;
  const int profile_waves = blocks * (grid.threads / 64);
  const size_t num_projected = r.projected.size();
  auto convert = [q, seg, na, agg_slot_of, lw, kernel_id, host_record, count_entries, count_leap2, profile_waves, num_projected](const BlockPartial& fp, pg_result* out) {
    out->num_aggregations = na;
    out->aggregations = (pg_agg_value*)calloc((size_t)std::max(na, 1), sizeof(pg_agg_value));
    for (int a = 0; a < na; ++a) {
      const pg_aggregation& ag = q->aggregations[a];
      pg_agg_value& v = out->aggregations[a];
      empty_agg_value(&v, (int64_t)fp.count);
      if (ag.function == PG_AGG_COUNT || ag.function == PG_AGG_DISTINCTCOUNT || ag.function == PG_AGG_PERCENTILE || is_hll_function(ag.function) || is_moments_function(ag.function)) continue;      // (a DISTINCTCOUNT's count is its bitset's: filled in behind the copy; a PERCENTILE's is the docs aggregated)
      const int ac = agg_slot_of[(size_t)a];
      const ColumnDev& col = seg->cols[(size_t)ag.column];
      const bool plane = lw.plane_cols[(size_t)ag.column] != 0;
      const bool raw = col.encoding == PG_FWD_RAW_FIXED_BYTE;
      if (ag.function == PG_AGG_SUM || ag.function == PG_AGG_AVG) {
        if (col.vkind == kValF64 || col.vkind == kValF32) {
          // SumAggregationFunction on FLOAT / DOUBLE: a double sum; the addition order differs from the reference's
          // doc order, so the last bits may (tests/test_gpu_typed.py states the tolerance)
          v.sum = fp.fsum[ac];
          v.sum_i64 = 0;
          v.sum_exact = 0;
        } else if (col.vkind == kValI64) {
          // LONG values: the int64 sum is exact unless it wrapped, which the double image of the same sum reveals (a wrap moves
          // it by a multiple of 2^64).  Wrapped: report the double sum, like the reference's double accumulation, inexact.
          v.sum_i64 = fp.sum[ac];
          const bool wrapped = std::fabs(fp.fsum[ac] - (double)fp.sum[ac]) > 4.6e18;
          v.sum_exact = wrapped ? 0 : 1;
          v.sum = wrapped ? fp.fsum[ac] : (double)v.sum_i64;
        } else {
          // value plane: sum(value) = count * base + sum(value - base); offset dictionaries add count * value_base
          set_integer_sum(&v, (__int128)fp.sum[ac] * (__int128)sum_scale(col, plane) + (__int128)fp.count * (__int128)sum_base(col, plane));
        }
      } else if (fp.count > 0) {
        if (raw && col.vkind != kValI32) {
          double mn = key64_to_double(col, fp.kmin64[ac]), mx = key64_to_double(col, fp.kmax64[ac]);
          if (mx != mx) mn = mx;      // Math.min / Math.max propagate NaN
          if (ag.function == PG_AGG_MIN) v.min = mn;
          if (ag.function == PG_AGG_MAX) v.max = mx;
        } else {
          if (ag.function == PG_AGG_MIN) v.min = agg_value_double(col, fp.kmin[ac], plane);
          if (ag.function == PG_AGG_MAX) v.max = agg_value_double(col, fp.kmax[ac], plane);
          // Math.min / Math.max propagate NaN: the largest dictId seen (every scan kernel folds it next to the smallest, whichever
          // the query asks for) tells a MIN that a doc with the NaN entry matched
          if (dict_ends_in_nan(col) && fp.kmax[ac] == col.cardinality - 1) {
            if (ag.function == PG_AGG_MIN) v.min = col.h_dict_f64.back();
          }
        }
      }
    }
    out->dominant_kernel = kernel_id;
    for (int c = 0; c < 4; ++c) out->profile_cycles[c] = fp.cyc[c];
    out->profile_waves = profile_waves;
    out->stats.num_docs_scanned = (int64_t)fp.count;
    // (the scan kernels count into their records; a leap-frogging a AND b adds what leapfrog2_chain_kernel left in the pinned record)
    finish_filter_stats(lw, seg, (int64_t)fp.entries + (count_leap2 ? host_record->leap_correction : 0), count_entries, out);
    out->stats.num_entries_scanned_post_filter = (int64_t)fp.count * (int64_t)num_projected;
    out->stats.num_total_docs = seg->num_docs;
  };
  // The workgroups' records are folded by the scan kernel's last workgroup, straight into the pinned host record.
  // Measured (profiles/r3, tools/ab_r3.py): the fold costs the kernel 5.5 us of tail on a 1024-workgroup grid where the finalize launch
  // costs 8.8 us (boundary + a one-workgroup kernel) -- 13 % of a 10 M-row query's device time.  Round 4: at EVERY size (1 B-row scans
  // were left with the separate launch so that the scan kernel's profiler duration was "the scan and nothing else"; the query paid
  // ~15 us for that, and its roofline fraction is a statement about the query, not about its largest kernel).
  const bool folded = g_engine.fold_finalize >= 0 ? g_engine.fold_finalize != 0 : true;
  sp.done_counter = folded ? ctx->d_done : nullptr;
  sp.host_out = g_engine.direct_result ? ctx->h_record_dev : nullptr;
  sp.host_seq = seq;
  // fields a fold reduces: the aggregation slots in use (the histogram kernel keeps its checksum in slot 1), typed extras only for the typed kernels
  sp.fold_slots = k.kernel == ScanKernel::Hist ? 2 : pl.num_agg_cols;
  sp.fold_typed = (k.kernel == ScanKernel::PrivateTyped || (k.kernel == ScanKernel::Agg && typed)) ? 1 : 0;
  sp.lane_skip = g_engine.lane_skip ? 1 : 0;
  sp.set_leaves_in_lds = 0;
  if (g_engine.set_lds) for (int nd = 0; nd < sp.num_nodes; ++nd) if (sp.nodes[nd].op == PG_FILTER_LEAF && sp.nodes[nd].kind == kLeafDictSet) sp.set_leaves_in_lds = 1;
  if (k.kernel == ScanKernel::Hist || pass.form != SetPass::None) sp.set_leaves_in_lds = grid.hist_set_off != 0 ? 1 + (int32_t)grid.hist_set_off : 0;      // (the histogram / set-pass kernels keep the area in their dynamic LDS, behind the counters / bitsets)
  if (pass.form != SetPass::None) { st = arm_set_pass(r, &pass, grid); if (st != PG_OK) return st; }
  sp.sparse_lanes = g_engine.sparse_lanes;
  sp.fold_one_counter = g_engine.fold_one_counter;
  if (defer_index_and) {
    auto item = index_and_item(lw);
    item->one_slot = pl.num_agg_cols <= 1;
    item->convert = convert;
    return defer_item(r, std::move(item));
  }
  // (the shared launch is for the many small segments of a server: a segment that fills the chip on its own -- more tiles than a few
  //  rounds of resident waves -- runs the kernel the planner picked for it, concurrently with the others, on a worker thread's stream:
  //  eight 1 B-row items 4.72 ms in one launch, 4.45 ms as eight overlapping launches)
  BatchKind kind = BatchKind::Private;
  if (r.defer != nullptr && !r.defer->single && scan_batch_kind(k, pl.num_agg_cols, &kind) && !want_bitmap && out && sp.tile_list == nullptr && !count_entries &&
      !ctx->pre_enqueued && g_engine.direct_result && lw.side == nullptr && doc_tiles(seg) <= kBatchMaxTiles && r.stats_is_final) {
    sp.lean_kind = (int32_t)kind;
    auto item = std::make_shared<LoweredItem>();
    item->sp = sp;
    item->blocks = blocks;
    item->one_slot = pl.num_agg_cols <= 1;
    item->convert = convert;
    item->sets = lw.set_leaves;
    if (k.kernel == ScanKernel::Hist) { item->hist_lds = grid.lds; item->hist_cw = k.hist_cw; item->hist_col = r.hist_col; }
    return defer_item(r, std::move(item));
  }
  // HIP events (PG_CFG_TIME_KERNELS): [ev_first, ev_last] brackets the query's device work, [ev[1], ev[2]] the scan kernel.  Each
  // record is a packet of its own on the queue, so a query that runs nothing but the scan kernel records just the two.
  // (the chain kernel / copy commands behind the scan kernel; a kernel that leaves leaf bitmaps behind for the transducer pass must have
  //  RETIRED before that pass reads them -- its plain stores are only ordered by the end of the kernel, not by the pinned record's seq)
  if (lw.gathered) {
    // index_and_kernel did the aggregation: its counter lines are the query's record
    // (timed runs: ev[0] in front of the kernel and ev[3] behind the copy, like the COUNT(*) path -- two more records between the
    //  kernel and its copy were two more packets on the queue, ~5 us that only a timed run paid)
    HIP_TRY(hipMemcpyAsync(ctx->h_and_shards, ctx->d_and_counters + 2, kAndShardBytes, hipMemcpyDeviceToHost, ctx->stream));
    if (timed) HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream));
    ctx->ev_last = 3;
    exec_mark(3);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    exec_mark(4);
    BlockPartial g;
    st = read_index_and_shards(ctx, pl.num_agg_cols, &g); if (st != PG_OK) return st;
    *ctx->h_partial = g;
  } else {
    // (the bitsets' copy follows the kernel on the stream: the polled record does not cover it)
    const bool post_work = !g_engine.direct_result || count_leap2 || want_bitmap || sp.leaf_out_enabled || k.kernel == ScanKernel::PrivateFsm || pass.form != SetPass::None;
    if (timed) HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
    if (pass.form != SetPass::None) launch_set_pass(r, &pass, grid);
    else launch_scan_kernel(k, grid, pl.num_agg_cols, typed, ctx->stream, sp);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(ctx->ev[2], ctx->stream));
    if (pass.form != SetPass::None) { st = enqueue_set_pass_post(r, &pass); if (st != PG_OK) return st; }
    if (!folded) {
      finalize_partials_kernel<<<dim3(1), dim3(kBlockThreads), 0, ctx->stream>>>(ctx->d_partials, blocks, g_engine.direct_result ? ctx->h_record_dev : nullptr, seq,
                                                                                  sp.fold_slots, sp.fold_typed, sp.profile);
      HIP_TRY(hipGetLastError());
    }
    if (!g_engine.direct_result) HIP_TRY(hipMemcpyAsync(ctx->h_partial, ctx->d_partials + blocks, sizeof(BlockPartial), hipMemcpyDeviceToHost, ctx->stream));
    if (count_leap2) { st = launch_leap_chain(seg, ctx, seq); if (st != PG_OK) return st; }
    if (k.kernel == ScanKernel::PrivateFsm) {
      // the tiles' tables -> the count (the same two kernels that end the separate pass), then eight bytes to the context's pinned counter
      const FsmSide& fs = *lw.side;
      fsm_chain_kernel<<<dim3((unsigned)fs.num_chunks), dim3(1024), 0, ctx->stream>>>(fs.tables, fs.num_tiles, sp.fsm_states, fs.chunks);
      HIP_TRY(hipGetLastError());
      fsm_finish_kernel<<<dim3(1), dim3(1024), (size_t)fs.num_chunks * (size_t)sp.fsm_states * 4, ctx->stream>>>(fs.chunks, (int)fs.num_chunks, sp.fsm_states, fs.entries);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(ctx->h_filter_entries, fs.entries, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (want_bitmap) {
      const int64_t need = ((int64_t)seg->num_docs + 63) / 64;
      if (d_out_bitmap_request) {
        if (need) HIP_TRY(hipMemcpyAsync(d_out_bitmap_request, ctx->d_bitmaps[0], (size_t)need * 8, hipMemcpyDeviceToDevice, ctx->stream));
      } else {
        if (host_bitmap_words < need) return fail(PG_ERR_INVALID_ARGUMENT, "bitmap buffer has %lld words, need %lld", (long long)host_bitmap_words, (long long)need);
        if (need) HIP_TRY(hipMemcpyAsync(host_bitmap, ctx->d_bitmaps[0], (size_t)need * 8, hipMemcpyDeviceToHost, ctx->stream));
      }
    }
    if (timed && (post_work || !folded)) HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream));
    ctx->ev_last = (post_work || !folded) ? 3 : 2;
    exec_mark(3);
    if (g_engine.poll_result && !post_work && !timed) {
      // nothing follows the kernel on the stream: the record's sequence number is the completion signal
      volatile unsigned long long* flag = &ctx->h_record->seq;
      st = wait_polled(ctx->stream, (long long)seg->num_docs, [&] { return *flag == seq; }); if (st != PG_OK) return st;
      if (*flag != seq) return fail(PG_ERR_INTERNAL, "the scan kernel finished without publishing its record");
    } else {
      HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    exec_mark(4);
    if (count_leap2 && ctx->h_record->leap_seq != seq) return fail(PG_ERR_INTERNAL, "the leap-frog chain kernel did not publish its result");
    if (g_engine.direct_result && ctx->h_record->seq != seq) return fail(PG_ERR_INTERNAL, "the scan kernel's record carries sequence %llu, expected %llu", ctx->h_record->seq, seq);
  }
  const BlockPartial& fp = *ctx->h_partial;
  // (the in-kernel fold orders the workgroups' records against their arrival counter through write-through stores, not through a
  //  release / acquire pair: every record carries its launch's stamp and a foreign one is an error, never an answer)
  if (fp.flags & kPartialStale) return fail(PG_ERR_INTERNAL, "the scan kernel's fold read a record that was not written by this launch (sequence %llu)", seq);
  // plain narrow counters: the counters must add up to the matches (a wrapped counter always leaves the total short)
  const bool hist_wrapped = k.kernel == ScanKernel::Hist && !k.hist_guarded && k.hist_cw < 32 && (unsigned long long)fp.sum[1] != fp.count;
  if (k.kernel == ScanKernel::Hist && (hist_wrapped || (fp.flags & kPartialHistAlarm))) {
    // Skewed dictIds: the histogram's sum is not used.  From now on the column runs in the next tier -- guarded counters, which count
    // hot dictIds exactly through guard-bit claims, then the value plane / gather path -- and execute_impl answers this query again.
    __atomic_store_n(&seg->cols[(size_t)r.hist_col].hist_tier, hist_wrapped ? 1 : 2, __ATOMIC_RELAXED);
    seg->plane_epoch.fetch_add(1, std::memory_order_acq_rel);      // (what the plan cache holds for this segment was lowered for the plain tier)
    return kHistRetry;
  }
  if (out_cardinality) *out_cardinality = (int64_t)fp.count;
  if (out) convert(fp, out);
  if (pass.form != SetPass::None) { st = harvest_set_pass(r, &pass, fp); if (st != PG_OK) return st; }
  if (out && k.kernel == ScanKernel::PrivateFsm) {
    // (the stream was synchronised: the walk's count is in the pinned counter)
    out->stats.num_entries_scanned_in_filter = (int64_t)*ctx->h_filter_entries;
    out->filter_entries_exact = 1;
    lw.side->fused = true;
  }
  return PG_OK;
}
// ---------------- group-by ----------------
// The kernel that aggregates a group-by, decided once (choose_group_route) and in this precedence: the partitioned passes
// (run_partitioned_group_by), group_typed_direct_kernel, group_private_kernel, scan_group_kernel.  DESIGN.md has the table.
enum class GroupRoute { Partition, TypedDirect, Private, Staged };
// What run_group_by's stages settle about a query before its first launch, beside the QueryRun
struct GroupPlan {
  GroupParams gp;
  std::vector<int> cards;                  // the key columns' cardinalities, in multiplier order
  int group_slot[kMaxGroupCols] = {}, group_mult[kMaxGroupCols] = {};
  PlanGroupAgg plan_aggs[kMaxGroupAggs];   // the distinct (column slot, SUM|MIN|MAX) pairs: the device's accumulators ...
  std::vector<int> dev_agg_of;             // ... and per aggregation of the query which of them it reads (-1: COUNT)
  HashPlan hash_plan; long long product = 1;      // product: raw keys (direct-indexed table), or the slots of a hashed one
  bool no_dict_keys = false;               // a key is a raw column read through its key image, or the null-key image of one
  bool first_appearance = false, map_based = false, private_leaves = true;      // private_leaves: every filter leaf is of a kind the lane-private filter implements
  size_t table_words = 0, table_bytes = 0; Geometry geo;      // geo: the staged launch (scan_group_kernel)
  int pblocks = 1, pthreads = kBlockThreads; size_t plds = 0;      // the private launch (group_private_kernel; also what the shared launch of a batch takes)
  PartitionPlan part; int packed_bits = 0;      // pg_group_plan.h; packed_bits: Partition's partition_packed_bits, else 0
  GroupRoute route = GroupRoute::Staged;
  bool count_leap2 = false, count_entries = false;      // arm_group_stats: the kernel counts numEntriesScannedInFilter
  GroupPlan() { memset(&gp, 0, sizeof(gp)); }
  // The launch was sized for group_private_kernel: a partitioned query passes every test of the private one (its first-doc pass and a batch go by that geometry)
  bool private_sized() const { return route == GroupRoute::Partition || route == GroupRoute::Private; }
  // The kernel evaluates the filter leaf by leaf over every doc: it can leave the leaves' outputs and entry counts behind.  NOT the condition under
  // which the index AND's bitmap must be complete: every route but Private reads that bitmap on every tile (arm_group_stats).
  bool route_writes_leaf_outputs() const { return route == GroupRoute::Private || route == GroupRoute::TypedDirect; }
  // pg_result.dominant_kernel.  group_typed_direct_kernel has no id of its own: such a query has always reported PG_KERNEL_SCAN_GROUP.
  int kernel_id() const { return route == GroupRoute::Partition ? PG_KERNEL_GROUP_PARTITION : (route == GroupRoute::Private ? PG_KERNEL_GROUP_PRIVATE : PG_KERNEL_SCAN_GROUP); }
};
// A raw key of a direct-indexed holder -> the dictIds of its columns (the first column is the least significant digit)
static inline void decode_mixed_radix(long long raw, const std::vector<int>& cards, int ng, int32_t* out) {
  for (int g = 0; g < ng; ++g) { out[g] = (int32_t)(raw % cards[(size_t)g]); raw /= cards[(size_t)g]; }
}
// One accumulator of one group -> the reference's holder value for aggregation `ag` (not COUNT) in *v, which already carries the group's count.
// `acc` is what the standalone kernels leave in the table; the shared launch of a batch removes its zero-identity bias first.  The floating-point and raw
// 8-byte branches are not reached from there: the deferral requires private_sized(), which implies dense_ok != 0, i.e. 32-bit-domain accumulators only.
static void group_agg_value(const pg_segment* seg, const pg_aggregation& ag, bool plane, long long acc, unsigned long long group_docs, pg_agg_value* v) {
  const ColumnDev& col = seg->cols[(size_t)ag.column];
  if (ag.function == PG_AGG_SUM || ag.function == PG_AGG_AVG) {
    if (col.vkind == kValF64 || col.vkind == kValF32) { memcpy(&v->sum, &acc, 8); v->sum_i64 = 0; v->sum_exact = 0; }      // the slot accumulated doubles (ds_add_f64 / global_atomic_add_f64)
    else set_integer_sum(v, (__int128)acc * (__int128)sum_scale(col, plane) + (__int128)group_docs * (__int128)sum_base(col, plane));
  }
  else if (col.encoding == PG_FWD_RAW_FIXED_BYTE && col.vkind != kValI32) {      // raw LONG value, or the order key of a raw FLOAT / DOUBLE value
    if (ag.function == PG_AGG_MIN) v->min = group_key64_to_double(col, acc, true); else v->max = group_key64_to_double(col, acc, false);
  }
  else if (ag.function == PG_AGG_MIN) v->min = group_dict_min_double(col, (int32_t)acc, plane);
  else v->max = agg_value_double(col, (int32_t)acc, plane);
}
// pg_execute_batch: a group-by of the LDS-table form over a small segment shares ONE launch with the batch's other such items
// (group_lds_batch_kernel; BatchKind::GroupLds) -- no table init, no compaction launches: the item's slice of the batch's table is
// all-zero before the launch (zero-identity keys), comes back whole in the batch's one copy, and the host keeps the slots whose
// count is not zero.  What GroupByCombineOperator.java:102-165 gets from one task per segment.
static pg_status defer_group_item(QueryRun& r, const GroupPlan& p) {
  pg_segment* seg = r.seg; const pg_query* q = r.q; const Lowered& lw = r.lw; const int na = r.na, ng = r.ng;
  const GroupParams& gp = p.gp;
  auto item = std::make_shared<LoweredItem>();
  item->gp = std::make_shared<GroupParams>(gp);
  item->gp->zero_identity = 1;
  item->gp->scan.lean_kind = (int32_t)BatchKind::GroupLds;
  item->sp.lean_kind = (int32_t)BatchKind::GroupLds;
  item->blocks = p.pblocks; item->group_threads = p.pthreads; item->group_lds = p.plds;
  item->group_table_words = ((size_t)gp.num_groups * (size_t)(1 + gp.num_group_aggs) + 31) & ~(size_t)31;      // (slices start on 256-byte boundaries)
  item->sets = lw.set_leaves;
  const int G = gp.num_groups, NA = gp.num_group_aggs;
  std::array<int, kMaxGroupAggs> kinds{};
  for (int a = 0; a < NA; ++a) kinds[(size_t)a] = gp.group_aggs[a].kind;
  const size_t num_projected = r.projected.size();
  // (captured by value and kept with the cached item: what the conversion needs of the lowering -- the planes its aggregations read through
  //  and the statistics plan -- not the whole Lowered with its index-AND parameter block: advisor, round 5; and of the plan, never the plan itself)
  const std::vector<char> plane_cols = lw.plane_cols; const fstats::Plan stats_plan = lw.stats_plan; const int stats_scan_leaves = lw.stats_scan_leaves;
  const std::vector<int> cards = p.cards, dev_agg_of = p.dev_agg_of; const bool no_dict_keys = p.no_dict_keys;
  item->convert_group = [q, seg, na, ng, cards, dev_agg_of, plane_cols, stats_plan, stats_scan_leaves, G, kinds, num_projected, no_dict_keys](const unsigned long long* table, pg_result* out) {
    int num_present = 0, k = 0; long long docs = 0;
    for (int g = 0; g < G; ++g) num_present += table[g] != 0ull ? 1 : 0;
    start_group_result(out, na, ng, num_present, PG_KERNEL_GROUP_PRIVATE, no_dict_keys ? groups_limit(q) : G, 0);
    for (int g = 0; g < G; ++g) {
      const unsigned long long group_docs = table[g];
      if (group_docs == 0ull) continue;
      docs += (long long)group_docs;
      out->group_ids[k] = g;
      decode_mixed_radix(g, cards, ng, out->group_key_dict_ids + (size_t)k * (size_t)ng);
      for (int a = 0; a < na; ++a) {
        const pg_aggregation& ag = q->aggregations[a];
        pg_agg_value& v = out->group_aggregations[(size_t)k * (size_t)na + (size_t)a];
        empty_agg_value(&v, (int64_t)group_docs);
        if (ag.function == PG_AGG_COUNT) continue;
        const int da = dev_agg_of[(size_t)a];
        long long acc = (long long)table[(size_t)G * (size_t)(1 + da) + (size_t)g];
        // zero-identity keys of the shared launch (group_private_body's flush): MIN travelled as 2^31 - v, MAX as v + 2^31 + 1
        if (kinds[(size_t)da] == kGroupMin) acc = 0x80000000ll - acc;
        else if (kinds[(size_t)da] == kGroupMax) acc = acc - 0x80000001ll;
        group_agg_value(seg, ag, plane_cols[(size_t)ag.column] != 0, acc, group_docs, &v);
      }
      ++k;
    }
    out->stats.num_docs_scanned = docs;
    finish_filter_stats(stats_plan, stats_scan_leaves, seg, 0, false, out);
    out->stats.num_entries_scanned_post_filter = docs * (int64_t)num_projected;
    out->stats.num_total_docs = seg->num_docs;
  };
  return defer_item(r, std::move(item));
}
// Key spaces above the LDS table: the docs are partitioned by key range first, then every partition is aggregated in LDS
// (pg_group_partition.h) instead of one global atomic per doc and aggregation.  p.part: P scatter partitions, fine partitions of 2^shift
// keys each; two levels when log2_fine_per_coarse > 0 (pass A scatters by coarse partition, group_repartition_*_kernel by fine partition).
// Where everything lies in the record buffer: PartitionLayout (pg_group_plan.h).
static pg_status run_partitioned_group_by(QueryRun& r, const GroupPlan& p) {
  pg_segment* seg = r.seg; const pg_query* q = r.q; ExecCtx* ctx = r.ctx; const int ng = r.ng;
  const GroupParams& gp = p.gp; const int P = (int)p.part.scatter_partitions, partition_shift = p.part.shift, log2_fine_per_coarse = p.part.log2_fine_per_coarse;
  const int scatter_shift = p.part.scatter_shift(), packed_bits = p.packed_bits;
  const PartitionLayout lay(P, (size_t)std::max(seg->num_tiles, 1) * 2048, gp.num_group_aggs, packed_bits, log2_fine_per_coarse, sizeof(PartitionWork), kRepartitionChunk);
  const int num_vals = lay.num_vals; const size_t fine_slots = lay.fine_slots, bytes = lay.bytes;
  auto u32_at = [&](size_t off) { return reinterpret_cast<uint32_t*>(ctx->d_partition + off); };                       // (after the allocation below)
  auto work_at = [&](size_t off) { return reinterpret_cast<PartitionWork*>(ctx->d_partition + off); };
  if (ctx->partition_capacity < bytes) {
    if (ctx->d_partition) (void)hipFree(ctx->d_partition);
    ctx->d_partition = nullptr; ctx->partition_capacity = 0;
    if (hipMalloc((void**)&ctx->d_partition, bytes) != hipSuccess) return fail(PG_ERR_OUT_OF_MEMORY, "partitioned group-by needs %zu bytes of record buffers", bytes);
    ctx->partition_capacity = bytes;
  }
  PartitionParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.gp = gp; pp.shift = scatter_shift; pp.num_partitions = P; pp.packed_bits = packed_bits;      // (two levels: pass 0 and pass A work on coarse partitions)
  pp.upper = u32_at(lay.off_upper);
  pp.cursor = u32_at(lay.off_cursor);
  pp.offsets = u32_at(lay.off_offsets);
  pp.work = work_at(lay.off_work);
  pp.part_key = u32_at(lay.off_key);
  for (int a = 0; a < gp.num_group_aggs; ++a) pp.part_val[a] = u32_at(lay.off_val + (size_t)a * lay.val_stride);
  HIP_TRY(hipMemsetAsync(ctx->d_partition, 0, lay.off_offsets, ctx->stream));          // upper and cursor
  const long long tiles2k = doc_tiles(seg);
  const int hist_blocks = grid_blocks(seg, tiles2k, 4, 6, false);
  std::vector<int> stats_key{scatter_shift};
  for (int g = 0; g < ng; ++g) stats_key.push_back(q->group_by_columns[g]);
  std::vector<uint32_t> upper;
  if (g_engine.partition_stats_cache) {
    std::lock_guard<std::mutex> lk(seg->partition_stats_mu);
    for (const auto& e : seg->partition_stats) if (e.first == stats_key) upper = e.second;
  }
  if ((int)upper.size() != P) {
    upper.assign((size_t)P, 0u);
    launch_group_partition_histogram(hist_blocks, ctx->stream, pp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(upper.data(), pp.upper, (size_t)P * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (g_engine.partition_stats_cache) {
      std::lock_guard<std::mutex> lk(seg->partition_stats_mu);
      if (seg->partition_stats.size() < 64) seg->partition_stats.emplace_back(stats_key, upper);
    }
  }
  std::vector<uint32_t> offsets((size_t)P + 1, 0u);
  std::vector<PartitionWork> work;
  unsigned long long total_upper = 0;
  for (int i = 0; i < P; ++i) total_upper += upper[(size_t)i];
  const uint32_t chunk = partition_chunk(total_upper, seg->num_cus, (unsigned long long)kPartitionChunk);
  for (int i = 0; i < P; ++i) {
    offsets[(size_t)i + 1] = offsets[(size_t)i] + upper[(size_t)i];
    for (uint32_t s0 = 0; s0 < upper[(size_t)i]; s0 += chunk) work.push_back(PartitionWork{i, s0, std::min<uint32_t>(chunk, upper[(size_t)i] - s0), 0u});
  }
  HIP_TRY(hipMemcpyAsync(ctx->d_partition + lay.off_offsets, offsets.data(), offsets.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (!work.empty()) HIP_TRY(hipMemcpyAsync(ctx->d_partition + lay.off_work, work.data(), work.size() * sizeof(PartitionWork), hipMemcpyHostToDevice, ctx->stream));
  const int scatter_bpc = packed_bits > 0 ? blocks_per_cu_group_partition_scatter_packed(P) : std::max(1, waves_group_partition_scatter() / 4);
  const int scatter_blocks = grid_blocks(seg, tiles2k, 4, scatter_bpc, false);
  launch_group_partition_scatter(scatter_blocks, ctx->stream, pp);
  HIP_TRY(hipGetLastError());
  std::vector<PartitionWork> chunks;
  if (lay.two_level && !work.empty()) {
    RepartitionParams rp;
    memset(&rp, 0, sizeof(rp));
    rp.src_key = pp.part_key; rp.dst_key = u32_at(lay.off_key2);
    for (int a = 0; a < num_vals; ++a) { rp.src_val[a] = pp.part_val[a]; rp.dst_val[a] = u32_at(lay.off_val2 + (size_t)a * lay.val_stride); }
    rp.coarse_offsets = pp.offsets; rp.coarse_cursor = pp.cursor;
    rp.fine_count = u32_at(lay.off_fine); rp.fine_cursor = rp.fine_count + fine_slots; rp.work_count = rp.fine_cursor + fine_slots;      // count | cursor | work_count (zeroed together), then offsets
    rp.fine_offsets = u32_at(lay.off_fine_offsets); rp.work = work_at(lay.off_work2); rp.chunks = work_at(lay.off_chunks);
    rp.num_coarse = P; rp.log2_fine_per_coarse = log2_fine_per_coarse; rp.fine_shift = partition_shift; rp.packed_bits = packed_bits; rp.num_vals = num_vals; rp.aggregate_chunk = chunk;
    for (int i = 0; i < P; ++i)
      for (uint32_t s0 = 0; s0 < upper[(size_t)i]; s0 += kRepartitionChunk) chunks.push_back(PartitionWork{i, s0, std::min<uint32_t>(kRepartitionChunk, upper[(size_t)i] - s0), 0u});
    HIP_TRY(hipMemsetAsync(ctx->d_partition + lay.off_fine, 0, lay.fine_zero_bytes, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->d_partition + lay.off_chunks, chunks.data(), chunks.size() * sizeof(PartitionWork), hipMemcpyHostToDevice, ctx->stream));
    launch_group_repartition((int)chunks.size(), ctx->stream, rp);
    HIP_TRY(hipGetLastError());
    // pass B over the fine partitions: the second buffer, the device-built work list (as many workgroups as it can have entries)
    PartitionParams fine = pp;
    fine.shift = partition_shift;
    fine.num_partitions = (int32_t)fine_slots;
    fine.cursor = rp.fine_cursor; fine.offsets = rp.fine_offsets;
    fine.work = rp.work; fine.work_count = rp.work_count;
    fine.part_key = rp.dst_key;
    for (int a = 0; a < num_vals; ++a) fine.part_val[a] = rp.dst_val[a];
    launch_group_partition_aggregate((int)lay.max_work2, ((size_t)p.part.entry_bytes) << partition_shift, ctx->stream, fine);
  } else if (!work.empty()) {
    launch_group_partition_aggregate((int)work.size(), ((size_t)p.part.entry_bytes) << partition_shift, ctx->stream, pp);
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));      // `offsets` / `work` / `chunks` are pageable host vectors: keep them alive until the copies ran
  return PG_OK;
}
// The groups that exist, in ascending raw-key order: (raw key, doc count, accumulators[a * num_present + k]), read through ids_of /
// counts_of / acc_of -- the vectors below, or the context's pinned staging.
struct PresentGroups {
  std::vector<unsigned long long> hash_keys;                    // hashed holders: the keys of the present slots ...
  std::vector<std::vector<unsigned long long>> hash_keys_lvl;    // ... and, per chained first table, the key behind the slot number a later key starts with
  std::vector<int32_t> ids; std::vector<unsigned long long> counts; std::vector<long long> acc;
  const int32_t* ids_of = nullptr; const unsigned long long* counts_of = nullptr; const long long* acc_of = nullptr;
  int num_present = 0; long long docs = 0;
};

// IntMapBasedHolder range: compact the HBM table on the device; honour numGroupsLimit the way the reference does
// (_globalGroupIdUpperBound = min(product, numGroupsLimit), DictionaryBasedGroupKeyGenerator.java:176).
static pg_status compact_map_groups(QueryRun& r, const GroupPlan& p, PresentGroups* found) {
  pg_segment* seg = r.seg; const pg_query* q = r.q; pg_result* out = r.out; ExecCtx* ctx = r.ctx; const bool timed = r.timed; const GroupParams& gp = p.gp; const HashPlan& hash_plan = p.hash_plan;
  pg_status st = PG_OK;
  const int limit = groups_limit(q);
  const long long bound = hash_plan.kind != 0 ? (long long)limit : std::min<long long>(p.product, limit);      // LongMap / ArrayMap holders: _globalGroupIdUpperBound = numGroupsLimit (:150-163)
  const int num_chunks = (int)(((long long)gp.num_groups + kGroupChunk - 1) / kGroupChunk);
  DeviceScratch scratch(ctx);
  uint32_t* d_chunk_counts = (uint32_t*)scratch.alloc((size_t)num_chunks * 4);
  uint32_t* d_chunk_offsets = (uint32_t*)scratch.alloc((size_t)(num_chunks + 1) * 4);
  unsigned long long* d_total_docs = (unsigned long long*)scratch.alloc(8);
  if (!d_chunk_counts || !d_chunk_offsets || !d_total_docs) return fail(PG_ERR_OUT_OF_MEMORY, "group-by compaction scratch");
  uint32_t* d_first_doc = nullptr;
  uint32_t max_first_doc = 0xFFFFFFFFu;
  auto count_groups = [&](bool with_docs, uint32_t* total) -> pg_status {
    if (with_docs) HIP_TRY(hipMemsetAsync(d_total_docs, 0, 8, ctx->stream));
    group_chunk_count_kernel<<<dim3((unsigned)num_chunks), dim3(256), 0, ctx->stream>>>(gp.table_count, d_first_doc, max_first_doc, gp.num_groups, d_chunk_counts,
                                                                                         with_docs ? d_total_docs : nullptr);
    group_chunk_scan_kernel<<<dim3(1), dim3(1024), 0, ctx->stream>>>(d_chunk_counts, num_chunks, d_chunk_offsets);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(total, d_chunk_offsets + num_chunks, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (!with_docs) HIP_TRY(hipStreamSynchronize(ctx->stream));      // (the first pass waits behind its doc total)
    return PG_OK;
  };
  uint32_t total = 0;
  unsigned long long total_docs = 0;
  st = count_groups(true, &total); if (st != PG_OK) return st;
  HIP_TRY(hipMemcpyAsync(&total_docs, d_total_docs, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (timed) HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  found->docs = (long long)total_docs;
  out->num_groups_limit_reached = (long long)total >= (long long)limit ? 1 : 0;      // GroupByOperator.java:114-115
  if ((long long)total > bound) {
    // More groups than the reference would have created: it hands out group ids in order of first appearance (docId order)
    // and drops the docs of later keys, so the survivors are the `bound` groups whose first doc comes earliest.
    unsigned long long* d_filter = nullptr;
    if (q->num_filter_nodes > 0 && hash_plan.kind == 0) {
      d_filter = (unsigned long long*)scratch.alloc((((size_t)seg->num_docs + 63) / 64 + 1) * 8);
      if (!d_filter) return fail(PG_ERR_OUT_OF_MEMORY, "group-by first-doc pass: filter bitmap");
      pg_query fq = *q;
      fq.num_aggregations = 0; fq.num_group_by = 0;
      st = execute_impl(seg, &fq, nullptr, d_filter, nullptr, 0, nullptr);      // stays on the device
      if (st != PG_OK) return st;
    }
    d_first_doc = (uint32_t*)scratch.alloc((size_t)gp.num_groups * 4);
    if (!d_first_doc) return fail(PG_ERR_OUT_OF_MEMORY, "group-by first-doc pass: %d slots", gp.num_groups);
    HIP_TRY(hipMemsetAsync(d_first_doc, 0xFF, (size_t)gp.num_groups * 4, ctx->stream));
    // The survivors are the distinct keys of a PREFIX of the matching docs -- the reference stops admitting keys at the doc
    // where the bound-th one appears.  With far more groups than the limit that prefix is short, so the docs are visited in
    // growing prefixes until `bound` keys have a first doc, not all of them.
    uint32_t seen = 0;
    long long done_docs = 0;
    long long step_docs = std::max<long long>(1 << 16, 4 * bound);
    if (hash_plan.kind != 0) {
      // hashed holders: the group-by kernel once more, in its first-doc mode (same filter, same keys, every key already has its slot)
      GroupParams fg = gp;
      fg.first_doc = d_first_doc;
      fg.scan.filter_entries = nullptr; fg.scan.leap_tables = nullptr;
      for (int n = 0; n < fg.scan.num_nodes; ++n) fg.scan.nodes[n].flags &= ~(kNodeLeapfrog2 | kNodeCountEntries);
      // (plds: the set area, when the filter has dictId sets.  A query whose aggregation runs in group_typed_direct_kernel never sized a
      //  group_private_kernel launch: the pass takes that kernel's own geometry then)
      const bool use_private = p.private_sized();
      const int fd_threads = use_private ? p.pthreads : kBlockThreads;
      const int fd_blocks = use_private ? p.pblocks : grid_blocks(seg, doc_tiles(seg), 4, 8, false);
      if (!use_private) fg.set_lds_off = -1;
      launch_group_private(false, fd_blocks, fd_threads, use_private ? p.plds : 0, ctx->stream, fg);
      HIP_TRY(hipGetLastError());
      done_docs = seg->num_docs;
      max_first_doc = 0xFFFFFFFEu;
      st = count_groups(false, &seen); if (st != PG_OK) return st;
    }
    while (done_docs < (long long)seg->num_docs && (long long)seen < bound) {
      const long long hi = std::min<long long>((long long)seg->num_docs, done_docs + step_docs);
      const long long span = hi - done_docs;
      group_first_doc_kernel<<<dim3((unsigned)std::min<long long>((span + 255) / 256, (long long)seg->num_cus * 16)), dim3(256), 0, ctx->stream>>>(gp, d_filter, d_first_doc, done_docs, hi);
      HIP_TRY(hipGetLastError());
      done_docs = hi;
      step_docs *= 2;
      max_first_doc = 0xFFFFFFFEu;            // "has a first doc"
      st = count_groups(false, &seen); if (st != PG_OK) return st;
    }
    uint32_t* d_present_first = (uint32_t*)scratch.alloc((size_t)std::max<uint32_t>(seen, 1) * 4);
    if (!d_present_first) return fail(PG_ERR_OUT_OF_MEMORY, "group-by first-doc pass: %u groups", seen);
    group_compact_kernel<<<dim3((unsigned)num_chunks), dim3(256), 0, ctx->stream>>>(gp.table_count, gp.table_acc, 0, gp.num_groups, d_first_doc, 0xFFFFFFFEu, d_chunk_offsets, seen,
                                                                                     nullptr, nullptr, nullptr, d_present_first);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> firsts((size_t)seen);
    HIP_TRY(hipMemcpyAsync(firsts.data(), d_present_first, (size_t)seen * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::nth_element(firsts.begin(), firsts.begin() + (bound - 1), firsts.end());
    max_first_doc = firsts[(size_t)bound - 1];      // first docs are distinct (a doc has one key): exactly `bound` groups pass
    st = count_groups(false, &total); if (st != PG_OK) return st;
  }
  found->num_present = (int)total;
  if (found->num_present > 0) {
    const size_t ids_bytes = ((size_t)found->num_present * 4 + 255) & ~(size_t)255, counts_bytes = (size_t)found->num_present * 8;
    const size_t acc_bytes = (size_t)found->num_present * (size_t)gp.num_group_aggs * 8;
    st = ensure_host_groups(ctx, ids_bytes + counts_bytes + acc_bytes + 256); if (st != PG_OK) return st;
    int32_t* h_ids = reinterpret_cast<int32_t*>(ctx->h_groups);
    unsigned long long* h_counts = reinterpret_cast<unsigned long long*>(ctx->h_groups + ids_bytes);
    long long* h_acc = reinterpret_cast<long long*>(ctx->h_groups + ids_bytes + counts_bytes);
    found->ids_of = h_ids; found->counts_of = h_counts; found->acc_of = h_acc;
    int32_t* d_ids = (int32_t*)scratch.alloc((size_t)found->num_present * 4);
    unsigned long long* d_counts = (unsigned long long*)scratch.alloc((size_t)found->num_present * 8);
    long long* d_acc = (long long*)scratch.alloc(std::max<size_t>((size_t)found->num_present * (size_t)gp.num_group_aggs * 8, 8));
    if (!d_ids || !d_counts || !d_acc) return fail(PG_ERR_OUT_OF_MEMORY, "group-by result of %d groups", found->num_present);
    group_compact_kernel<<<dim3((unsigned)num_chunks), dim3(256), 0, ctx->stream>>>(gp.table_count, gp.table_acc, gp.num_group_aggs, gp.num_groups, d_first_doc, max_first_doc,
                                                                                     d_chunk_offsets, total, d_ids, d_counts, d_acc, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_ids, d_ids, (size_t)found->num_present * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_counts, d_counts, counts_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (gp.num_group_aggs > 0) HIP_TRY(hipMemcpyAsync(h_acc, d_acc, acc_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (hash_plan.kind != 0) {
      // the slots that hold a group -> their 64-bit keys (and, for a key beyond a long, the first table's key behind its slot number)
      unsigned long long* d_keys = (unsigned long long*)scratch.alloc((size_t)found->num_present * 8 * (size_t)(1 + hash_plan.levels));
      if (!d_keys) return fail(PG_ERR_OUT_OF_MEMORY, "group-by keys of %d groups", found->num_present);
      found->hash_keys.resize((size_t)found->num_present);
      const unsigned gblocks = (unsigned)std::min<long long>(((long long)found->num_present + 255) / 256, (long long)seg->num_cus * 8);
      gather_u64_kernel<<<dim3(gblocks), dim3(256), 0, ctx->stream>>>(gp.hash_keys, d_ids, found->num_present, gp.hash_mask, d_keys);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(found->hash_keys.data(), d_keys, (size_t)found->num_present * 8, hipMemcpyDeviceToHost, ctx->stream));
      // chained first tables, last one first: the low part of a key is the slot number of the table before it
      found->hash_keys_lvl.resize((size_t)hash_plan.levels);
      for (int l = hash_plan.levels - 1; l >= 0; --l) {
        unsigned long long* src = d_keys + (size_t)(hash_plan.levels - 1 - l) * (size_t)found->num_present;
        found->hash_keys_lvl[(size_t)l].resize((size_t)found->num_present);
        gather_u64_by_key_kernel<<<dim3(gblocks), dim3(256), 0, ctx->stream>>>(gp.hash_keys_lvl[l], src, found->num_present, gp.hash_mask_lvl[l], src + found->num_present);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(found->hash_keys_lvl[(size_t)l].data(), src + found->num_present, (size_t)found->num_present * 8, hipMemcpyDeviceToHost, ctx->stream));
      }
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  return PG_OK;
}
// The stages of run_group_by, in call order; their declines keep the order they had in one function (a query with two problems gets the first's message).
// plan, 1: the key columns' streams, the holder (direct-indexed or hashed), the key space
static pg_status bind_group_keys(QueryRun& r, GroupPlan* p) {
  pg_segment* seg = r.seg; const pg_query* q = r.q; Lowered& lw = r.lw; PlanParams& pl = lw.plan; const int ng = r.ng, num_cols_total = (int)seg->cols.size();
  const HashPlan& hash_plan = p->hash_plan;
  pg_status st = PG_OK;
  for (int g = 0; g < ng; ++g) {
    int c = q->group_by_columns[g];
    if (c < 0 || c >= num_cols_total) return fail(PG_ERR_INVALID_ARGUMENT, "group-by column %d out of range", c);
    r.add_projected(seg->cols[(size_t)c].key_image_of >= 0 ? seg->cols[(size_t)c].key_image_of : c);      // numEntriesScannedPostFilter counts the caller's column
    if (seg->cols[(size_t)c].encoding != PG_FWD_FIXED_BIT_DICT) {
      // NoDictionarySingle/MultiColumnGroupKeyGenerator: the raw INT / LONG column through its key image (value - min as the dictId)
      st = ensure_key_image(seg, c, &c); if (st != PG_OK) return st;
    }
    const ColumnDev& col = seg->cols[(size_t)c];
    p->no_dict_keys |= col.key_image_of >= 0;
    int s = slot_for(&lw, seg, c);
    if (s < 0) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
    pl.cols[s].in_agg = 1;
    p->group_slot[g] = s;
    p->cards.push_back(col.cardinality);
  }
  // DictionaryBasedGroupKeyGenerator.java:164-184: up to arrayBasedThreshold (10 000) the raw key IS the group id (ArrayBasedHolder);
  // above it the reference hashes raw keys (IntMapBasedHolder) -- here the table stays direct-indexed, in HBM, one slot per raw
  // key, and only the groups that exist come back.  2^24 slots keep the 24-bit key multiplies exact and the table <= 1.2 GB.
  // Beyond an int (Long / ArrayMap holders) the table is hashed: `product` is then its number of slots (plan_hash_holder).
  st = plan_hash_holder(seg, p->cards, &p->hash_plan); if (st != PG_OK) return st;
  if (hash_plan.kind == 0) {
    for (int g = 0; g < ng; ++g) { p->group_mult[g] = (int32_t)p->product; p->product *= p->cards[(size_t)g]; }
  } else {
    p->product = hash_plan.slots;
    if (q->flags & kQueryHashHolder) return fail(PG_ERR_UNSUPPORTED, "group-by with raw keys beyond an int under null handling (plan-time fallback)");
  }
  // (kQueryHashHolder: the no-dictionary key generators of null handling hand out group ids by first appearance up to numGroupsLimit
  //  whatever the key space: the compaction path below is the one that honours the limit)
  // A raw key column always runs the no-dictionary generators (DefaultGroupByExecutor.java:106-121): _globalGroupIdUpperBound =
  // numGroupsLimit whatever the key space (NoDictionarySingleColumnGroupKeyGenerator.java:73-79), ids by first appearance.
  p->first_appearance = (q->flags & kQueryHashHolder) != 0 || (p->no_dict_keys && hash_plan.kind == 0 && (long long)groups_limit(q) < p->product);
  p->map_based = p->product > 10000 || p->first_appearance || hash_plan.kind != 0;
  p->gp.num_group_cols = ng;
  p->gp.num_groups = (int32_t)p->product;
  p->gp.dense_ok = 1;
  return PG_OK;
}
// plan, 2: the aggregations' columns, and the distinct accumulators the device keeps for them
static pg_status bind_group_aggs(QueryRun& r, GroupPlan* p) {
  pg_segment* seg = r.seg; const pg_query* q = r.q; Lowered& lw = r.lw; PlanParams& pl = lw.plan; const int na = r.na, num_cols_total = (int)seg->cols.size();
  GroupParams& gp = p->gp; PlanGroupAgg* plan_aggs = p->plan_aggs; std::vector<int>& dev_agg_of = p->dev_agg_of;
  dev_agg_of.assign((size_t)std::max(na, 1), -1);
  for (int a = 0; a < na; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    if (ag.function == PG_AGG_COUNT) {
      if ((q->flags & kQueryCountReadsColumn) && ag.column >= 0 && ag.column < num_cols_total) r.add_projected(ag.column);
      continue;
    }
    if (ag.function < PG_AGG_COUNT || ag.function > PG_AGG_AVG) return fail(PG_ERR_UNSUPPORTED, "aggregation function %d", ag.function);
    if (ag.column < 0 || ag.column >= num_cols_total) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation column %d out of range", ag.column);
    r.add_projected(ag.column);
    if (ag.function == PG_AGG_MAX && dict_ends_in_nan(seg->cols[(size_t)ag.column])) return fail_group_max_over_nan_dictionary(seg->cols[(size_t)ag.column].name.c_str());
    int s = slot_for(&lw, seg, ag.column, lw.plane_cols[(size_t)ag.column] != 0);
    if (s < 0) return fail(PG_ERR_UNSUPPORTED, "query references more than %d columns", kMaxCols);
    pl.cols[s].in_agg = 1;
    const int kind = (ag.function == PG_AGG_SUM || ag.function == PG_AGG_AVG) ? kGroupSum : (ag.function == PG_AGG_MIN ? kGroupMin : kGroupMax);
    int da = -1;
    for (int i = 0; i < gp.num_group_aggs; ++i) if (plan_aggs[i].col == s && plan_aggs[i].kind == kind) da = i;
    if (da < 0) {
      if (gp.num_group_aggs >= kMaxGroupAggs) return fail(PG_ERR_UNSUPPORTED, "more than %d distinct group-by aggregations", kMaxGroupAggs);
      da = gp.num_group_aggs++;
      plan_aggs[da] = PlanGroupAgg{s, kind};
    }
    dev_agg_of[(size_t)a] = da;
  }
  gp.wide_keys = p->product > (1ll << 24) ? 1 : 0;
  return PG_OK;
}
// plan, 3: the table -- count[G] | acc[num_group_aggs][G], behind them a hashed holder's keys and first tables -- in the context's d_table; the columns' place in a staged tile
static pg_status lay_out_group_table(QueryRun& r, GroupPlan* p) {
  pg_segment* seg = r.seg; ExecCtx* ctx = r.ctx; Lowered& lw = r.lw; ScanParams& sp = lw.sp; PlanParams& pl = lw.plan; const int ng = r.ng;
  GroupParams& gp = p->gp; const HashPlan& hash_plan = p->hash_plan; const PlanGroupAgg* plan_aggs = p->plan_aggs; Geometry& geo = p->geo;
  // (hashed holders: one more word per slot for its key, and the first table of an ArrayMap-range key)
  p->table_words = (size_t)gp.num_groups * (size_t)(1 + gp.num_group_aggs + (hash_plan.kind ? 1 : 0)) + (size_t)hash_plan.level_slots(); p->table_bytes = p->table_words * 8;
  if ((unsigned long long)p->table_words * 8ull > g_engine.group_table_bytes)
    return fail(PG_ERR_UNSUPPORTED, "group-by table of %lld slots x %d words exceeds the %llu-byte budget (PINOT_GPU_GROUP_TABLE_BYTES)", p->product, 1 + gp.num_group_aggs,
                (unsigned long long)g_engine.group_table_bytes);
  const pg_status st = ensure_table(ctx, p->table_words, p->map_based ? 0 : p->table_words); if (st != PG_OK) return st;
  gp.table_count = ctx->d_table; gp.table_acc = reinterpret_cast<long long*>(ctx->d_table + gp.num_groups);
  gp.hash_kind = hash_plan.kind; gp.hash_levels = hash_plan.levels;
  if (hash_plan.kind != 0) {
    gp.hash_mask = (unsigned long long)gp.num_groups - 1ull;
    gp.hash_keys = ctx->d_table + (size_t)gp.num_groups * (size_t)(1 + gp.num_group_aggs);
    unsigned long long* next_table = gp.hash_keys + gp.num_groups;
    for (int l = 0; l < hash_plan.levels; ++l) {
      gp.hash_split[l] = hash_plan.split[l]; gp.hash_mask_lvl[l] = (unsigned long long)hash_plan.slots_lvl[l] - 1ull;
      gp.hash_keys_lvl[l] = next_table; next_table += hash_plan.slots_lvl[l];
    }
    for (int g = 0; g < ng; ++g) gp.key_mult[g] = hash_plan.mult[g];
  }
  // the staged geometry (which places the column streams), then the keys and accumulators as the kernels read them
  const int group_wave_cap = waves_scan_group();
  finish_geometry(seg, &lw, p->table_bytes, false, g_engine.group_waves > 0 ? std::min(g_engine.group_waves, kGroupBlockThreads / 64) : kGroupBlockThreads / 64, group_wave_cap, &geo);
  if ((size_t)sp.wave_lds_bytes > kLdsBudget) return fail(PG_ERR_UNSUPPORTED, "query needs %d bytes of LDS per wavefront", sp.wave_lds_bytes);
  gp.use_lds_table = geo.table_in_lds ? 1 : 0;
  sp.speculate = 1;
  for (int g = 0; g < ng; ++g) { const DevColumn& c = pl.cols[p->group_slot[g]]; gp.group_keys[g] = DevGroupKey{c.bits, c.slot_off, p->group_mult[g], 0, c.fwd}; }
  for (int a = 0; a < gp.num_group_aggs; ++a) {
    const DevColumn& c = pl.cols[plan_aggs[a].col];
    DevGroupAgg& ga = gp.group_aggs[a];
    ga.kind = plan_aggs[a].kind; ga.bits = c.bits; ga.slot_off = c.slot_off; ga.is_raw = c.is_raw; ga.is_plane = c.is_plane;
    ga.dict_bytes = c.dict_bytes; ga.fwd = c.fwd; ga.dict = c.dict;
    // MIN / MAX run on dictIds whatever the value type; only a SUM reads 8-byte / floating-point dictionary entries
    ga.vkind = (ga.kind == kGroupSum) ? c.vkind : kValI32;
    if (c.is_raw && c.vkind != kValI32) ga.vkind = c.vkind;      // group_typed_direct_kernel: the value type decides the accumulator
    if (ga.vkind != kValI32) gp.dense_ok = 0;
    if (ga.vkind == kValI64 && !c.is_raw) {
      // the table slot is one wrapping int64: refuse (plan-time fallback) when numDocs * max|value| could overflow it
      const ColumnDev& sc = seg->cols[(size_t)(lw.col_of_slot[(size_t)plan_aggs[a].col] / 2)];
      const double max_abs = std::max(std::fabs((double)sc.h_dict_i64.front()), std::fabs((double)sc.h_dict_i64.back()));
      if ((double)seg->num_docs * max_abs >= 9.2e18) return fail(PG_ERR_UNSUPPORTED, "group-by SUM of LONG column %s could overflow int64", sc.name.c_str());
    }
  }
  return PG_OK;
}
// plan, 4: the route
static pg_status choose_group_route(QueryRun& r, GroupPlan* p) {
  const pg_segment* seg = r.seg; const PlanParams& pl = r.lw.plan; const bool want_bitmap = r.want_bitmap; const GroupParams& gp = p->gp; const HashPlan& hash_plan = p->hash_plan;
  // An accumulator is a raw LONG / FLOAT / DOUBLE value: group_typed_direct_kernel.  So is the SUM of a dictionary column with 8-byte values under a Long /
  // ArrayMap holder: the staged kernel that gathers such values has no hashed table, group_typed_direct_kernel<.., kHash> gathers them too.
  bool typed_direct = false;
  for (int a = 0; a < gp.num_group_aggs; ++a) typed_direct |= gp.group_aggs[a].vkind != kValI32 && (gp.group_aggs[a].is_raw || hash_plan.kind != 0);
  // Without a filter every tile is aggregated in full: the lane-private kernel decodes straight from HBM and needs LDS only
  // for the table (group_private_kernel).
  // every leaf kind the lane-private filter implements (scan / set / bitmap / docId-range leaves, raw INT ranges)
  bool& private_leaves = p->private_leaves;
  for (int l = 0; l < pl.num_leaves; ++l) private_leaves &= pl.leaves[l].kind <= kLeafBitmap || pl.leaves[l].kind == kLeafDocRange;
  if (typed_direct && !private_leaves) return fail(PG_ERR_UNSUPPORTED, "group-by aggregation of a raw 8-byte column under a raw 8-byte range predicate (plan-time fallback)");
  const bool use_private = (g_engine.group_private || hash_plan.kind != 0) && private_leaves && gp.dense_ok && !want_bitmap && !typed_direct;
  if (hash_plan.kind != 0 && !use_private && !typed_direct) return fail(PG_ERR_UNSUPPORTED, "group-by with raw keys beyond an int: only 32-bit-domain or raw 8-byte aggregations under lane-private filter leaves");
  // Key spaces above the LDS table: partition the docs by key range first, then aggregate every partition in LDS (pg_group_partition.h) instead of one
  // global atomic per doc and aggregation.  More fine partitions than one scatter pass can address (key spaces of 2 M .. 2^31 raw keys): two levels
  // (partition_plan, pg_group_plan.h).  PINOT_GPU_PARTITION_TWO_LEVEL=0: such key spaces keep the direct HBM atomics.
  p->part = partition_plan(p->product, gp.num_group_aggs, kMaxPartitions);
  const bool use_partition = hash_plan.kind == 0 && !typed_direct && p->map_based && g_engine.group_partition && g_engine.group_private && private_leaves && gp.dense_ok && !want_bitmap &&
                             gp.num_group_aggs <= kMaxPartitionAggs && (!p->part.two_level() || (g_engine.partition_two_level && (1 << p->part.log2_fine_per_coarse) <= kMaxFinePerCoarse)) &&
                             (long long)seg->num_docs >= g_engine.partition_min_docs;
  p->route = use_partition ? GroupRoute::Partition : (typed_direct ? GroupRoute::TypedDirect : (use_private ? GroupRoute::Private : GroupRoute::Staged));
  const DevGroupAgg& ga = gp.group_aggs[0];
  if (use_partition) p->packed_bits = partition_packed_bits(g_engine.partition_packed, gp.num_group_aggs, ga.kind == kGroupSum, ga.bits, ga.is_raw != 0, ga.is_plane != 0, ga.vkind == kValI32, p->part.scatter_shift());
  return PG_OK;
}
// plan, 5: the private launch, count packing, the LDS table's replicas and the set area; the scan block the kernels get
static pg_status size_group_launch(QueryRun& r, GroupPlan* p) {
  pg_segment* seg = r.seg; ExecCtx* ctx = r.ctx; Lowered& lw = r.lw; ScanParams& sp = lw.sp; GroupParams& gp = p->gp; const Geometry& geo = p->geo;
  const size_t table_bytes = p->table_bytes; const bool use_private = p->private_sized(); const int blocks = geo.blocks;
  // the private launch: the staged geometry unless the route is sized for group_private_kernel
  int& pblocks = p->pblocks; int& pthreads = p->pthreads; size_t& plds = p->plds;
  pblocks = blocks;
  pthreads = geo.threads;
  plds = geo.lds;
  if (use_private) {
    const int private_wave_cap = waves_group_private();
    const bool in_lds = table_bytes <= 96 * 1024; gp.use_lds_table = in_lds ? 1 : 0;
    int waves = in_lds ? kGroupBlockThreads / 64 : kBlockThreads / 64;
    if (g_engine.group_waves > 0) waves = std::min(waves, g_engine.group_waves);
    while (waves > private_wave_cap) waves >>= 1;
    pthreads = waves * 64; plds = in_lds ? table_bytes : 0;
    int bpc = std::max(1, private_wave_cap / waves);
    if (in_lds) bpc = std::max(1, std::min(bpc, (int)(kLdsBudget / std::max<size_t>(plds, 1))));
    pblocks = grid_blocks(seg, doc_tiles(seg), waves, bpc);
  }
  // Count packing (count_bits / count_packed_shift, pg_group_plan.h): the first summed value plane that is narrow enough for the docs a
  // workgroup sees carries the count in its LDS slot.
  gp.packed_agg = -1; gp.packed_shift = 0;
  if (gp.use_lds_table && g_engine.group_pack) {
    const long long waves_total = use_private ? (long long)pblocks * (pthreads / 64) : (long long)blocks * (geo.threads / 64);
    const long long tiles_total = use_private ? doc_tiles(seg) : (long long)sp.num_tiles;
    const long long tiles_per_wave = (tiles_total + waves_total - 1) / waves_total;
    const long long docs_per_block = use_private ? tiles_per_wave * (pthreads / 64) * 2048 : tiles_per_wave * (geo.threads / 64) * 64 * sp.tile_steps;
    const int cbits = count_bits(docs_per_block);
    for (int a = 0; a < gp.num_group_aggs; ++a) {
      const DevGroupAgg& ga = gp.group_aggs[a];
      const int shift = (ga.kind == kGroupSum && ga.is_plane && !ga.is_raw) ? count_packed_shift(cbits, ga.bits) : 0;
      if (shift != 0) { gp.packed_agg = a; gp.packed_shift = shift; break; }
    }
  }
  // group_private_kernel's LDS table in as many bank-interleaved copies as the workgroup's share of the CU's LDS holds (pg_kernels.h,
  // lds_group_table_bytes): C3's 1000 groups x (SUM + MAX) are 12 KB a copy, eight copies for the one 16-wave workgroup of a CU.
  gp.lds_log_replicas = 0;
  // (a filter with dictId-set leaves: kSetLdsWords words of the workgroup's LDS hold the sets, behind the table -- pg_kernels.h stage_filter_sets)
  sp.set_leaves_in_lds = 0;
  if (g_engine.set_lds) for (int nd = 0; nd < sp.num_nodes; ++nd) if (sp.nodes[nd].op == PG_FILTER_LEAF && sp.nodes[nd].kind == kLeafDictSet) sp.set_leaves_in_lds = 1;
  const size_t set_area = (use_private && sp.set_leaves_in_lds != 0) ? (size_t)kSetLdsWords * 4 : 0;
  if (use_private && gp.use_lds_table) {
    const int resident = std::max(1, std::min(waves_group_private() / std::max(1, pthreads / 64), g_engine.blocks_per_cu > 0 ? g_engine.blocks_per_cu : 1 << 30));
    const size_t budget = kLdsBudget / (size_t)resident - set_area;
    int log_r = 0;
    while (log_r < g_engine.group_log_replicas && (size_t)lds_group_table_bytes(gp, log_r + 1) <= budget) ++log_r;
    gp.lds_log_replicas = log_r; plds = lds_group_table_bytes(gp, log_r);
  }
  gp.set_lds_off = -1;
  if (set_area != 0 && plds + set_area <= kLdsBudget) { gp.set_lds_off = (int32_t)((plds + 15) & ~(size_t)15); plds = (size_t)gp.set_lds_off + set_area; }
  gp.scan = sp;
  gp.scan.partials = nullptr;
  gp.scan.out_bitmap = nullptr;
  if (lw.tile_list != nullptr) { const pg_status st = complete_index_list(&lw, ctx); if (st != PG_OK) return st; }
  gp.scan.tile_list = lw.tile_list; gp.scan.tile_count = lw.tile_count;            // read by group_private_kernel only
  gp.scan.filter_entries = nullptr;
  return PG_OK;
}
// run, 1: the table's identities; PINOT_GPU_PARTITION_TRACE's line
static pg_status init_group_table(QueryRun& r, const GroupPlan& p) {
  const pg_segment* seg = r.seg; ExecCtx* ctx = r.ctx; const GroupParams& gp = p.gp;
  HIP_TRY(mark_pre_work(ctx));
  init_group_table_kernel<<<dim3((unsigned)std::max<long long>(64, std::min<long long>(p.product >> 12, (long long)seg->num_cus * 16))), dim3(256), 0, ctx->stream>>>(gp);
  HIP_TRY(hipGetLastError());
  if (r.timed) HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
  static const bool partition_trace = getenv("PINOT_GPU_PARTITION_TRACE") != nullptr;
  if (partition_trace)
    fprintf(stderr, "group-by plan: product %lld, fine partitions %lld (shift %d), 2^%d per coarse -> %lld scatter partitions; partition %d (hash %d typed_direct %d map_based %d "
                    "private_leaves %d dense_ok %d aggs %d docs %d packed_bits %d)\n", p.product, p.part.fine_partitions, p.part.shift, p.part.log2_fine_per_coarse, p.part.scatter_partitions,
            (int)(p.route == GroupRoute::Partition), p.hash_plan.kind, (int)(p.route == GroupRoute::TypedDirect), (int)p.map_based, (int)p.private_leaves, gp.dense_ok, gp.num_group_aggs,
            seg->num_docs, p.packed_bits);
  return PG_OK;
}
// run, 2: what the filter statistics need of the kernel -- the leaves' outputs for the transducer pass, the leapfrog tables, the entry counter
static pg_status arm_group_stats(QueryRun& r, GroupPlan* p) {
  pg_segment* seg = r.seg; pg_result* out = r.out; ExecCtx* ctx = r.ctx; Lowered& lw = r.lw; GroupParams& gp = p->gp; pg_status st = PG_OK;
  // (every kernel but group_private_kernel walks EVERY tile and reads the index AND's bitmap there: the tiles the AND did not list must be zero,
  //  not what an earlier query of this context left in them -- only group_private_kernel goes by the tile list.  Not route_writes_leaf_outputs().)
  if (p->route != GroupRoute::Private) { st = complete_index_and_bitmap(&lw, ctx); if (st != PG_OK) return st; }
  if (lw.side != nullptr) {
    const bool wrote = p->route_writes_leaf_outputs() && gp.scan.tile_list == nullptr;
    for (int l = 0; l < kMaxLeaves; ++l) gp.scan.leaf_out[l] = wrote ? lw.sp_leaf_out[l] : nullptr;
    gp.scan.leaf_out_enabled = wrote ? 1 : 0;
    lw.side->kernel_wrote = wrote;
  }
  const bool count_leap2 = p->count_leap2 = out && lw.stats_leap2_flagged && p->route_writes_leaf_outputs();
  const bool count_entries = p->count_entries = (out && lw.stats_chain_flagged && p->route_writes_leaf_outputs()) || count_leap2;
  gp.scan.leap_tables = nullptr;
  if (count_leap2) { st = arm_leap_tables(seg, ctx, &gp.scan.leap_tables, &gp.scan.filter_entries); if (st != PG_OK) return st; }
  else if (lw.stats_leap2_flagged) for (int n = 0; n < gp.scan.num_nodes; ++n) gp.scan.nodes[n].flags &= ~kNodeLeapfrog2;
  if (count_entries && !count_leap2) { st = arm_filter_entries(ctx, &gp.scan.filter_entries); if (st != PG_OK) return st; }
  return PG_OK;
}
// run, 3: the route's kernel(s), and behind them what the entry count needs on the stream
static pg_status launch_group_route(QueryRun& r, const GroupPlan& p) {
  pg_segment* seg = r.seg; ExecCtx* ctx = r.ctx; const GroupParams& gp = p.gp; pg_status st = PG_OK;
  switch (p.route) {
    case GroupRoute::Partition: st = run_partitioned_group_by(r, p); if (st != PG_OK) return st; break;
    case GroupRoute::TypedDirect: launch_group_typed_direct(grid_blocks(seg, doc_tiles(seg), 4, 8, false), ctx->stream, gp); break;
    case GroupRoute::Private: launch_group_private(gp.use_lds_table != 0, p.pblocks, p.pthreads, p.plds, ctx->stream, gp); break;
    case GroupRoute::Staged: launch_scan_group(g_engine.use_dma, gp.use_lds_table != 0, p.geo.blocks, p.geo.threads, p.geo.lds, ctx->stream, gp); break;
  }
  HIP_TRY(hipGetLastError());
  if (r.timed) HIP_TRY(hipEventRecord(ctx->ev[2], ctx->stream));
  if (p.count_leap2) { st = launch_leap_chain(seg, ctx, 0); if (st != PG_OK) return st; }
  if (p.count_entries) HIP_TRY(hipMemcpyAsync(ctx->h_filter_entries, ctx->d_filter_entries, 8, hipMemcpyDeviceToHost, ctx->stream));
  return PG_OK;
}
// run, 4: the groups that exist, in ascending raw-key order (hashed holders: in slot order)
static pg_status harvest_groups(QueryRun& r, const GroupPlan& p, PresentGroups* found_out) {
  ExecCtx* ctx = r.ctx; const bool timed = r.timed; const GroupParams& gp = p.gp; PresentGroups& found = *found_out;
  if (!p.map_based) {
    HIP_TRY(hipMemcpyAsync(ctx->h_table, ctx->d_table, p.table_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (timed) HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const unsigned long long* hc = ctx->h_table; const long long* ha = reinterpret_cast<const long long*>(ctx->h_table + gp.num_groups);
    for (int g = 0; g < gp.num_groups; ++g) if (hc[g]) { found.num_present++; found.docs += (long long)hc[g]; }
    found.ids.reserve((size_t)found.num_present); found.counts.reserve((size_t)found.num_present); found.acc.resize((size_t)found.num_present * (size_t)gp.num_group_aggs);
    int k = 0;
    for (int g = 0; g < gp.num_groups; ++g) {
      if (!hc[g]) continue;
      found.ids.push_back(g); found.counts.push_back(hc[g]);
      for (int a = 0; a < gp.num_group_aggs; ++a) found.acc[(size_t)a * (size_t)found.num_present + (size_t)k] = ha[(size_t)a * (size_t)gp.num_groups + (size_t)g];
      k++;
    }
  } else {
    const pg_status st = compact_map_groups(r, p, &found); if (st != PG_OK) return st;
  }
  if (!found.ids_of) { found.ids_of = found.ids.data(); found.counts_of = found.counts.data(); found.acc_of = found.acc.data(); }
  return PG_OK;
}
// result, 1: the header, and the keys as dictId tuples for every kind of holder (what GroupKeyGenerator.getGroupKeys turns into values); rows in ascending raw-key order.
// hashed holders / no-dictionary generators: group_id_upper_bound = numGroupsLimit, like the reference (:150-163); out of the table in slot order, `perm` sorts them.
static void decode_group_keys(QueryRun& r, const GroupPlan& p, const PresentGroups& found, std::vector<int>* perm_out) {
  pg_result* out = r.out; const int ng = r.ng; const HashPlan& hash_plan = p.hash_plan; const std::vector<int>& cards = p.cards; std::vector<int>& perm = *perm_out;
  start_group_result(out, r.na, ng, found.num_present, p.kernel_id(), (hash_plan.kind != 0 || p.no_dict_keys) ? groups_limit(r.q) : p.gp.num_groups, hash_plan.kind);
  if (hash_plan.kind == 0) {
    for (int k = 0; k < found.num_present; ++k) decode_mixed_radix(found.ids_of[(size_t)k], cards, ng, out->group_key_dict_ids + (size_t)k * (size_t)ng);
  } else {
    std::vector<int32_t> tuples((size_t)found.num_present * (size_t)ng);
    for (int k = 0; k < found.num_present; ++k) {
      // key l covers the columns [segment_begin(l), segment_end(l)); above its lowest digit -- the slot number of table l - 1 -- it is
      // a mixed-radix number of those columns' dictIds
      for (int l = 0; l <= hash_plan.levels; ++l) {
        unsigned long long key = l == hash_plan.levels ? found.hash_keys[(size_t)k] : found.hash_keys_lvl[(size_t)l][(size_t)k];
        if (l > 0) key /= (unsigned long long)hash_plan.slots_lvl[l - 1];
        for (int g = hash_plan.segment_begin(l); g < hash_plan.segment_end(l, ng); ++g) {
          tuples[(size_t)k * (size_t)ng + (size_t)g] = (int32_t)(key % (unsigned long long)cards[(size_t)g]); key /= (unsigned long long)cards[(size_t)g];
        }
      }
    }
    perm.resize((size_t)found.num_present);
    for (int k = 0; k < found.num_present; ++k) perm[(size_t)k] = k;
    std::sort(perm.begin(), perm.end(), [&](int a, int b) {
      for (int g = ng - 1; g >= 0; --g) {      // the last column is the most significant digit of the raw key
        const int32_t x = tuples[(size_t)a * (size_t)ng + (size_t)g], y = tuples[(size_t)b * (size_t)ng + (size_t)g];
        if (x != y) return x < y;
      }
      return false;
    });
    if (hash_plan.kind == 1) out->group_ids64 = (int64_t*)malloc(sizeof(int64_t) * (size_t)std::max(found.num_present, 1));
    for (int k = 0; k < found.num_present; ++k) {
      const int src = perm[(size_t)k];
      memcpy(out->group_key_dict_ids + (size_t)k * (size_t)ng, tuples.data() + (size_t)src * (size_t)ng, sizeof(int32_t) * (size_t)ng);
      if (hash_plan.kind == 1) out->group_ids64[k] = (int64_t)found.hash_keys[(size_t)src];
    }
  }
}
// result, 2: the rows' holder values, and the statistics.  Turning accumulators into the reference's holder values is independent per group: large results
// (the IntMapBasedHolder range returns up to numGroupsLimit rows) are converted by a few host threads, each touching its own pages of the result.
static void convert_group_rows(QueryRun& r, const GroupPlan& p, const PresentGroups& found, const std::vector<int>& perm) {
  const pg_segment* seg = r.seg; const pg_query* q = r.q; pg_result* out = r.out; ExecCtx* ctx = r.ctx; const Lowered& lw = r.lw; const int na = r.na; const std::vector<int>& dev_agg_of = p.dev_agg_of;
  auto convert_groups = [&](int k_begin, int k_end) {
  for (int k = k_begin; k < k_end; ++k) {
    const int src = perm.empty() ? k : perm[(size_t)k];       // the row of the compacted table behind result row k
    const unsigned long long group_docs = found.counts_of[(size_t)src];
    out->group_ids[k] = perm.empty() ? found.ids_of[(size_t)src] : k;      // (hashed holders: a row number; the key is in group_ids64 / group_key_dict_ids)
    for (int a = 0; a < na; ++a) {
      const pg_aggregation& ag = q->aggregations[a];
      pg_agg_value& v = out->group_aggregations[(size_t)k * (size_t)na + (size_t)a];
      empty_agg_value(&v, (int64_t)group_docs);
      if (ag.function == PG_AGG_COUNT) continue;
      const long long acc = found.acc_of[(size_t)dev_agg_of[(size_t)a] * (size_t)found.num_present + (size_t)src];
      group_agg_value(seg, ag, lw.plane_cols[(size_t)ag.column] != 0, acc, group_docs, &v);
    }
  }
  };
  const int convert_threads = found.num_present >= (1 << 16) ? (int)std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency())) : 1;
  if (convert_threads <= 1) convert_groups(0, found.num_present);
  else {
    std::vector<std::thread> workers;
    for (int t = 0; t < convert_threads; ++t) {
      const int k0 = (int)((long long)found.num_present * t / convert_threads), k1 = (int)((long long)found.num_present * (t + 1) / convert_threads);
      workers.emplace_back(convert_groups, k0, k1);
    }
    for (auto& w : workers) w.join();
  }
  out->stats.num_docs_scanned = found.docs;
  finish_filter_stats(lw, seg, p.count_entries ? (int64_t)*ctx->h_filter_entries : 0, p.count_entries, out);
  out->stats.num_entries_scanned_post_filter = found.docs * (int64_t)r.projected.size();
  out->stats.num_total_docs = seg->num_docs;
}
// DictionaryBasedGroupKeyGenerator's holders: plan (GroupPlan), then either hand the query to a batch's shared launch or run its route and
// turn the table into the result.
static pg_status run_group_by(QueryRun& r) {
  GroupPlan p; PresentGroups found; std::vector<int> perm; pg_status st = PG_OK;
  // a table of the upper IntMapBasedHolder range goes back to the allocator with the query.  (Armed before lay_out_group_table, the only caller of
  // ensure_table, so that every exit behind the allocation trims: no table above the bound outlives its query, and the guard finds none on entry.)
  struct TableTrim {
    ExecCtx* c;
    ~TableTrim() { if (c->table_capacity * 8 > kGroupTableKeepBytes) { (void)hipFree(c->d_table); c->d_table = nullptr; c->table_capacity = 0; } }
  } table_trim{r.ctx};
  if ((st = bind_group_keys(r, &p)) != PG_OK || (st = bind_group_aggs(r, &p)) != PG_OK || (st = lay_out_group_table(r, &p)) != PG_OK ||
      (st = choose_group_route(r, &p)) != PG_OK || (st = size_group_launch(r, &p)) != PG_OK) return st;
  const Lowered& lw = r.lw;
  if (r.defer != nullptr && g_engine.batch_group && p.private_sized() && p.gp.use_lds_table && p.hash_plan.kind == 0 && !p.first_appearance && !r.want_bitmap && r.out &&
      lw.tile_list == nullptr && lw.side == nullptr && !lw.stats_leap2_flagged && !lw.stats_chain_flagged && !r.ctx->pre_enqueued && r.stats_is_final &&
      (long long)groups_limit(r.q) >= p.product && (r.defer->single || doc_tiles(r.seg) <= kBatchMaxTiles))
    return defer_group_item(r, p);
  if ((st = init_group_table(r, p)) != PG_OK || (st = arm_group_stats(r, &p)) != PG_OK || (st = launch_group_route(r, p)) != PG_OK || (st = harvest_groups(r, p, &found)) != PG_OK) return st;
  decode_group_keys(r, p, found, &perm);
  convert_group_rows(r, p, found, perm);
  return PG_OK;
}
// The query's device time (PG_CFG_TIME_KERNELS) and the transducer pass behind its kernels
static pg_status finish_query(QueryRun& r) {
  pg_segment* seg = r.seg; const pg_query* q = r.q; pg_result* out = r.out; ExecCtx* ctx = r.ctx; const Lowered& lw = r.lw; const bool timed = r.timed;
  if (timed && out && lw.gathered) { const pg_status st = time_index_and(ctx, out); if (st != PG_OK) return st; }
  else if (timed && out) {
    float ms_all = 0.f, ms_scan = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms_scan, ctx->ev[1], ctx->ev[2]));
    if (!ctx->pre_started && ctx->ev_last == 2) ms_all = ms_scan;
    else HIP_TRY(hipEventElapsedTime(&ms_all, ctx->ev[ctx->pre_started ? 0 : 1], ctx->ev[ctx->ev_last]));
    out->device_ms = ms_all;
    out->dominant_kernel_ms = ms_scan;
    if (ctx->pre_started && lw.tile_list != nullptr) {
      // index-led query: when the index phase (index_and_kernel + its finalize) outlasts the scan of the listed tiles, IT is the dominant kernel
      float ms_index = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms_index, ctx->ev[0], ctx->ev[1]));
      if (ms_index > ms_scan) { out->dominant_kernel = PG_KERNEL_INDEX_AND; out->dominant_kernel_ms = ms_index; }
    }
  }
  if (out && lw.side != nullptr && !lw.side->fused && !out->filter_entries_exact) {
    // The transducer pass (pg_filter_fsm.h) behind the query's own kernels: they have retired (the result above was read), the leaves' bitmaps
    // they left are in this context's scratch, the context is still ours.  A pass that fails leaves the answer standing, inexact.
    if (device_fsm_filter_stats(seg, ctx, q, *lw.side, out) != PG_OK) { (void)hipGetLastError(); out->filter_entries_exact = 0; }
  }
  return PG_OK;
}
static pg_status execute_impl(pg_segment* seg, const pg_query* q, pg_result* out, unsigned long long* d_out_bitmap_request,
                              uint64_t* host_bitmap, int64_t host_bitmap_words, int64_t* out_cardinality, bool allow_metadata_plan,
                              Deferred* defer, FsmSide* side) {
  if (!g_engine.initialized) return fail(PG_ERR_NOT_INITIALIZED, "pg_init has not been called");
  if (!seg || !q) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  // d_out_bitmap_request: like host_bitmap, but the filter's doc-order bitmap is copied device to device into the caller's
  // buffer ((num_docs + 63) / 64 words, any stream-ordered device memory) and never visits the host.
  {
    pg_query shape = *q;                      // pg_filter_bitmap evaluates the filter only
    if (host_bitmap != nullptr || d_out_bitmap_request != nullptr) { shape.num_aggregations = 0; shape.num_group_by = 0; }
    const pg_status eligible = check_query_plan(seg, &shape, 0);
    if (eligible != PG_OK) return eligible;
  }
  exec_mark(1);
  HIP_TRY(hipSetDevice(phys_device(seg->device)));
  ExecCtx* ctx = nullptr;
  pg_status st = acquire_ctx(seg, &ctx); if (st != PG_OK) return st;
  CtxGuard guard{seg, ctx};

  const bool want_bitmap = host_bitmap != nullptr || d_out_bitmap_request != nullptr;
  const int na = want_bitmap ? 0 : q->num_aggregations;
  const int ng = (want_bitmap || (q->flags & kQuerySetPass)) ? 0 : q->num_group_by;      // (the bitset pass of a DISTINCTCOUNT query is an aggregation-only launch: its group-by columns are the kernel's keys)
  if (na < 0 || ng < 0 || (na > 0 && !q->aggregations) || (ng > 0 && !q->group_by_columns)) return fail(PG_ERR_INVALID_ARGUMENT, "bad aggregation / group-by lists");
  if ((q->flags & kQuerySetPass) && !want_bitmap && (q->num_group_by < 0 || (q->num_group_by > 0 && !q->group_by_columns))) return fail(PG_ERR_INVALID_ARGUMENT, "bad aggregation / group-by lists");
  if (ng > kMaxGroupCols) return fail(PG_ERR_UNSUPPORTED, "more than %d group-by columns", kMaxGroupCols);
  const bool timed = (g_engine.flags & PG_CFG_TIME_KERNELS) != 0;
  if (ng == 0 && !want_bitmap && out && na > 0 && allow_metadata_plan && answer_from_metadata(seg, q, na, out, out_cardinality)) return PG_OK;
  if (ng == 0 && !want_bitmap && out && na > 0 && answer_from_doc_set(seg, q, na, out, out_cardinality)) return PG_OK;

  QueryRun r(seg, q, out, ctx, defer, na, ng, want_bitmap, timed);
  Lowered& lw = r.lw;
  memset(&lw.sp, 0, sizeof(lw.sp));
  memset(&lw.plan, 0, sizeof(lw.plan));
  lw.plan.lazy_node = -1;
  const int num_cols_total = (int)seg->cols.size();
  // Columns that are summed are read through their value plane (built on first use); decided before the filter is
  // lowered so that a range predicate on the same column can be evaluated on the plane too.
  lw.plane_cols.assign((size_t)std::max(num_cols_total, 1), 0);
  // At most one summed column goes through the LDS histogram instead (scan_hist_kernel); it needs the lane-private kernel, so the
  // shapes that kernel does not take are ruled out here, before a plane is (not) built.
  if (ng == 0 && !want_bitmap && g_engine.scan_private && !(g_engine.flags & PG_CFG_PROFILE_WAVES)) {
    bool shape_ok = true;
    int only_col = -1;                  // the histogram kernel aggregates ONE column (SUM / AVG / MIN / MAX of it, and COUNT)
    for (int a = 0; a < na && shape_ok; ++a) {
      const pg_aggregation& ag = q->aggregations[a];
      if (ag.function == PG_AGG_COUNT) continue;
      shape_ok = ag.column >= 0 && ag.column < num_cols_total && seg->cols[(size_t)ag.column].encoding == PG_FWD_FIXED_BIT_DICT &&
                 seg->cols[(size_t)ag.column].vkind == kValI32 && (only_col < 0 || only_col == ag.column);
      only_col = ag.column;
    }
    for (int i = 0; i < q->num_predicates && shape_ok && q->predicates; ++i) {
      const pg_predicate& pr = q->predicates[i];
      if (pr.kind == PG_PRED_RAW_RANGE) shape_ok = pr.column >= 0 && pr.column < num_cols_total && seg->cols[(size_t)pr.column].stored_type == PG_TYPE_INT;
    }
    for (int a = 0; a < na && shape_ok && r.hist_col < 0; ++a) {
      const pg_aggregation& ag = q->aggregations[a];
      if ((ag.function == PG_AGG_SUM || ag.function == PG_AGG_AVG) && want_hist(seg->cols[(size_t)ag.column])) r.hist_col = ag.column;
    }
  }
  for (int a = 0; a < na; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    if ((ag.function == PG_AGG_SUM || ag.function == PG_AGG_AVG) && ag.column >= 0 && ag.column < num_cols_total && ag.column != r.hist_col &&
        (want_value_plane(seg->cols[(size_t)ag.column]) || (!want_bitmap && want_wide_plane(seg, q, ag.column)))) {
      if (lw.plane_cols[(size_t)ag.column]) continue;
      bool ready = false;
      st = acquire_plane(seg, ag.column, &ready); if (st != PG_OK) return st;
      if (ready) { r.planes.columns.push_back(ag.column); lw.plane_cols[(size_t)ag.column] = 1; }
      else lw.plane_pending = true;
    }
  }
  ctx->pre_enqueued = false;
  ctx->pre_started = false;      // ev[0] is recorded by the first piece of work that precedes the scan kernel (mark_pre_work)
  ctx->ev_last = 3;
  if (out && !want_bitmap) lw.stats_plan = fstats::choose_plan(q, &lw.stats_scan_leaves);
  if (lw.stats_plan == fstats::Plan::kLeap2 && (!g_engine.leap2 || (q->flags & PG_QUERY_STATS_UPPER_BOUND_OK))) lw.stats_plan = fstats::Plan::kReplay;      // (kReplay with nobody replaying: the upper bound)
  // the caller takes the upper bound (PG_QUERY_STATS_UPPER_BOUND_OK): a leap-frogging filter has no pass behind its kernel, so in a batch it shares the launch like any other
  r.stats_is_final = lw.stats_plan == fstats::Plan::kZero || lw.stats_plan == fstats::Plan::kPerLeaf ||
                              (lw.stats_plan == fstats::Plan::kReplay && (q->flags & PG_QUERY_STATS_UPPER_BOUND_OK) != 0);
  lw.cardinality_only_hint = ng == 0 && out && !want_bitmap && na > 0;
  for (int a = 0; a < na; ++a) lw.cardinality_only_hint = lw.cardinality_only_hint && q->aggregations[a].function == PG_AGG_COUNT;
  lw.side = nullptr;
  if (out && !want_bitmap && lw.stats_plan == fstats::Plan::kReplay && side != nullptr && side->fsm != nullptr) {
    // numEntriesScannedInFilter is a statistic: a pass that cannot get its scratch leaves the query's answer standing with
    // filter_entries_exact = 0 (pg_execute's host replay still applies at its sizes) -- it never fails the query
    if (prepare_fsm_side(seg, ctx, *side->fsm, side) == PG_OK) lw.side = side;
    else (void)hipGetLastError();
  }
  // (never a value pass: PERCENTILE / DISTINCTCOUNT of ONE raw INT column behind ONE IN list has that shape too, and scan_raw_set_kernel collects nothing --
  //  the pass's kernels evaluate the lane-private filter, where a raw-set leaf is a pre-pass bitmap)
  lw.raw_set_lean_hint = lw.side == nullptr && (q->flags & kQuerySetPass) == 0 && raw_set_lean_shape(seg, q, na, ng, want_bitmap, out != nullptr);
  st = lower_filter(seg, ctx, q, &lw); if (st != PG_OK) return st;
  exec_mark(2);
  if (out) memset(out, 0, sizeof(*out));
  if (lw.cardinality_only_hint && lw.index_and_is_whole_filter) return count_from_index(r, out_cardinality);
  st = ng == 0 ? run_aggregation(r, d_out_bitmap_request, host_bitmap, host_bitmap_words, out_cardinality) : run_group_by(r);
  if (st == kHistRetry) {
    // (the histogram's next tier: the context goes back before the query is answered again)
    release_ctx(seg, ctx);
    guard.ctx = nullptr;
    return execute_impl(seg, q, out, d_out_bitmap_request, host_bitmap, host_bitmap_words, out_cardinality, allow_metadata_plan, nullptr, side);
  }
  if (st != PG_OK) return st;
  return finish_query(r);
}

// ---- PG_QUERY_NULL_HANDLING (query option enableNullHandling=true) ----
// The reference gives every filter operator three docId sets -- trues, nulls, falses (BaseFilterOperator.java:85-113) -- and the
// aggregation functions skip the null docs of their own column (NullableSingleInputAggregationFunction.java:72-166).  Both are
// lowered HERE, on the host, into plain two-valued work for the kernels: the filter becomes an ordinary tree whose extra leaves
// read the columns' null bitmaps (IS_NULL postings expanded at open), and the aggregations are split into one lane per nullable
// column, each lane running the filter AND "column IS NOT NULL".  The kernels do not know about nulls.
struct FilterExpr {
  int op = PG_FILTER_LEAF;
  pg_predicate pred{};
  std::vector<FilterExpr> kids;
};

struct NullRewriter {
  const pg_segment* seg;
  bool has_nulls(int column) const { return column >= 0 && column < (int)seg->cols.size() && seg->cols[(size_t)column].d_null_bitmap != nullptr; }
  static bool column_leaf(const pg_predicate& p) {
    return p.kind == PG_PRED_DICT_RANGE || p.kind == PG_PRED_DICT_SET || p.kind == PG_PRED_RAW_RANGE || p.kind == PG_PRED_RAW_SET || p.kind == PG_PRED_DOC_RANGE;
  }
  static FilterExpr leaf(const pg_predicate& p) { FilterExpr e; e.pred = p; return e; }
  static FilterExpr null_leaf(int column, bool is_not_null) {
    pg_predicate p{};
    p.kind = PG_PRED_IS_NULL; p.column = column; p.exclusive = is_not_null ? 1 : 0;
    return leaf(p);
  }
  static FilterExpr combine(int op, std::vector<FilterExpr> kids) {
    if (kids.size() == 1 && op != PG_FILTER_NOT) return std::move(kids[0]);
    FilterExpr e; e.op = op; e.kids = std::move(kids);
    return e;
  }
  static FilterExpr negate(FilterExpr e) { std::vector<FilterExpr> k; k.push_back(std::move(e)); return combine(PG_FILTER_NOT, std::move(k)); }

  // getTrues(): BaseColumnFilterOperator.java:45-53 (matches AND NOT nulls); And / Or: of the children's trues; Not: the child's falses
  FilterExpr trues(const FilterExpr& e) const {
    if (e.op == PG_FILTER_LEAF) {
      if (column_leaf(e.pred) && has_nulls(e.pred.column)) return combine(PG_FILTER_AND, {leaf(e.pred), null_leaf(e.pred.column, true)});
      return e;
    }
    if (e.op == PG_FILTER_NOT) return falses(e.kids[0]);
    std::vector<FilterExpr> k;
    for (const auto& c : e.kids) k.push_back(trues(c));
    return combine(e.op, std::move(k));
  }
  // trues OR nulls of a child, as And / OrFilterOperator.getFalses collect them (AndFilterOperator.java:62-80): only column leaves
  // have a null set (BaseColumnFilterOperator.getNulls :56-64); (matches AND NOT nulls) OR nulls == matches OR nulls
  FilterExpr trues_or_nulls(const FilterExpr& e) const {
    if (e.op == PG_FILTER_LEAF && column_leaf(e.pred) && has_nulls(e.pred.column))
      return combine(PG_FILTER_OR, {leaf(e.pred), null_leaf(e.pred.column, false)});
    return trues(e);
  }
  // getFalses(): leaf NOT (trues OR nulls) (BaseFilterOperator.java:96-113); And / Or: NOT AND / OR of (trues_i OR nulls_i); Not: child trues
  FilterExpr falses(const FilterExpr& e) const {
    if (e.op == PG_FILTER_LEAF) return negate(trues_or_nulls(e));
    if (e.op == PG_FILTER_NOT) return trues(e.kids[0]);
    std::vector<FilterExpr> k;
    for (const auto& c : e.kids) k.push_back(trues_or_nulls(c));
    return negate(combine(e.op, std::move(k)));
  }
};

struct FlatQuery {
  std::vector<pg_filter_node> nodes;
  std::vector<pg_predicate> preds;
  std::vector<pg_aggregation> aggs;
  pg_query q{};
  void emit(const FilterExpr& e) {
    pg_filter_node n{};
    n.op = e.op;
    if (e.op == PG_FILTER_LEAF) { n.predicate = (int32_t)preds.size(); preds.push_back(e.pred); }
    else { for (const auto& c : e.kids) emit(c); n.predicate = -1; n.num_children = (int32_t)e.kids.size(); }
    nodes.push_back(n);
  }
  void finish(const pg_query& base) {
    q = base;
    q.flags = (base.flags & ~PG_QUERY_NULL_HANDLING) | ((base.flags & PG_QUERY_NULL_HANDLING) ? kQueryCountReadsColumn : 0);
    q.filter = nodes.empty() ? nullptr : nodes.data(); q.num_filter_nodes = (int32_t)nodes.size();
    q.predicates = preds.empty() ? nullptr : preds.data(); q.num_predicates = (int32_t)preds.size();
  }
};

static pg_status parse_filter(const pg_query* q, FilterExpr* root, bool* has_filter) {
  *has_filter = q->num_filter_nodes > 0;
  if (!*has_filter) return PG_OK;
  if (!q->filter || !q->predicates) return fail(PG_ERR_INVALID_ARGUMENT, "filter nodes without predicates");
  std::vector<FilterExpr> stack;
  for (int n = 0; n < q->num_filter_nodes; ++n) {
    const pg_filter_node& fn = q->filter[n];
    FilterExpr e;
    e.op = fn.op;
    if (fn.op == PG_FILTER_LEAF) {
      if (fn.predicate < 0 || fn.predicate >= q->num_predicates) return fail(PG_ERR_INVALID_ARGUMENT, "filter node %d: bad predicate index", n);
      e.pred = q->predicates[fn.predicate];
    } else if (fn.op == PG_FILTER_AND || fn.op == PG_FILTER_OR || fn.op == PG_FILTER_NOT) {
      const int k = fn.op == PG_FILTER_NOT ? 1 : fn.num_children;
      if (k < 1 || (int)stack.size() < k) return fail(PG_ERR_INVALID_ARGUMENT, "malformed filter tree (node %d)", n);
      e.kids.assign(std::make_move_iterator(stack.end() - k), std::make_move_iterator(stack.end()));
      stack.resize(stack.size() - (size_t)k);
    } else {
      return fail(PG_ERR_INVALID_ARGUMENT, "unknown filter op %d", fn.op);
    }
    stack.push_back(std::move(e));
  }
  if (stack.size() != 1) return fail(PG_ERR_INVALID_ARGUMENT, "malformed filter tree (%d roots)", (int)stack.size());
  *root = std::move(stack[0]);
  return PG_OK;
}

static pg_status execute_null_handling(pg_segment* seg, const pg_query* q, pg_result* out, uint64_t* host_bitmap, int64_t host_bitmap_words,
                                       int64_t* out_cardinality) {
  if (!seg || !q) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  NullRewriter rw{seg};
  FilterExpr root, filter_trues;
  bool has_filter = false;
  pg_status st = parse_filter(q, &root, &has_filter);
  if (st != PG_OK) return st;
  if (has_filter) filter_trues = rw.trues(root);
  FlatQuery base;
  if (has_filter) base.emit(filter_trues);
  base.finish(*q);
  if (host_bitmap) return execute_impl(seg, &base.q, nullptr, nullptr, host_bitmap, host_bitmap_words, out_cardinality);
  const int na = q->num_aggregations, ng = q->num_group_by;
  if (na < 0 || ng < 0 || (na > 0 && !q->aggregations) || (ng > 0 && !q->group_by_columns)) return fail(PG_ERR_INVALID_ARGUMENT, "bad aggregation / group-by lists");
  // lanes: the nullable columns that are aggregated, in first-use order (AggregationPlanNode.hasNullValues :130-152)
  std::vector<int> lane_cols;
  for (int a = 0; a < na; ++a) {
    const int c = q->aggregations[a].column;
    if (rw.has_nulls(c) && std::find(lane_cols.begin(), lane_cols.end(), c) == lane_cols.end()) lane_cols.push_back(c);
  }
  if (ng > 0) {
    // DefaultGroupByExecutor.java:106-121: under null handling the keys come from the no-dictionary generators -- NULL is a key value of
    // its own -- and every aggregation function skips the null docs of its own column (NullableSingleInputAggregationFunction
    // .aggregateGroupBySV :118-160).  Here: a nullable key column is read through its null-key image (dictId = cardinality where the doc
    // is null: one more digit value of the raw group id), and the aggregations are split into lanes like above -- the base lane over the
    // filter's trues (COUNT(*) and the columns without nulls; it also decides which groups exist), one lane per nullable aggregated
    // column over trues AND column IS NOT NULL, merged by group id.  A group none of whose docs has a value in a lane comes back with
    // count 0 for that function: the reference's holder stays null.
    bool nullable_keys = false;
    std::vector<int32_t> keys((size_t)ng);
    for (int g = 0; g < ng; ++g) {
      const int c = q->group_by_columns[g];
      keys[(size_t)g] = c;
      if (!rw.has_nulls(c)) continue;
      if (seg->cols[(size_t)c].nullkey_column < 0) return fail(PG_ERR_UNSUPPORTED, "GROUP BY over nullable raw column %s keeps the CPU plan", seg->cols[(size_t)c].name.c_str());
      keys[(size_t)g] = seg->cols[(size_t)c].nullkey_column;
      nullable_keys = true;
    }
    base.q.group_by_columns = keys.data();
    if (nullable_keys || !lane_cols.empty()) {
      // numGroupsLimit binds at any key-space size here (NoDictionary*GroupKeyGenerator: _globalGroupIdUpperBound = numGroupsLimit)
      long long product = 1;
      for (int g = 0; g < ng; ++g) product *= std::max(seg->cols[(size_t)keys[(size_t)g]].cardinality, 1);
      const long long limit = groups_limit(q);
      if (limit < product) base.q.flags |= kQueryHashHolder;
    }
    if (lane_cols.empty()) return execute_impl(seg, &base.q, out, nullptr, nullptr, 0, nullptr);
    std::vector<int> base_pos;
    for (int a = 0; a < na; ++a) if (!rw.has_nulls(q->aggregations[a].column)) { base.aggs.push_back(q->aggregations[a]); base_pos.push_back(a); }
    const bool synthetic_count = base.aggs.empty();
    if (synthetic_count) base.aggs.push_back(pg_aggregation{PG_AGG_COUNT, -1});
    base.q.aggregations = base.aggs.data(); base.q.num_aggregations = (int32_t)base.aggs.size();
    pg_result part;
    memset(&part, 0, sizeof(part));
    st = execute_impl(seg, &base.q, &part, nullptr, nullptr, 0, nullptr, false);
    if (st != PG_OK) { pg_result_free(&part); return st; }
    memset(out, 0, sizeof(*out));
    const int num_groups = part.num_groups;
    const int base_na = part.num_aggregations;
    out->num_aggregations = na;
    out->num_groups = num_groups;
    out->group_id_upper_bound = part.group_id_upper_bound;
    out->num_groups_limit_reached = part.num_groups_limit_reached;
    out->stats = part.stats;
    out->filter_entries_exact = 0;
    out->device_ms = part.device_ms; out->dominant_kernel_ms = part.dominant_kernel_ms; out->dominant_kernel = part.dominant_kernel;
    out->group_ids = (int32_t*)malloc(sizeof(int32_t) * (size_t)std::max(num_groups, 1));
    out->group_aggregations = (pg_agg_value*)calloc((size_t)std::max(num_groups, 1) * (size_t)std::max(na, 1), sizeof(pg_agg_value));
    for (int k = 0; k < num_groups; ++k) {
      out->group_ids[k] = part.group_ids[k];
      for (int a = 0; a < na; ++a) {                       // until a lane says otherwise: no value reached the holder
        pg_agg_value& v = out->group_aggregations[(size_t)k * (size_t)na + (size_t)a];
        v.min = std::numeric_limits<double>::infinity();
        v.max = -std::numeric_limits<double>::infinity();
      }
      if (!synthetic_count) for (size_t i = 0; i < base_pos.size(); ++i) out->group_aggregations[(size_t)k * (size_t)na + (size_t)base_pos[i]] = part.group_aggregations[(size_t)k * (size_t)base_na + i];
    }
    out->group_key_kind = part.group_key_kind;
    out->group_key_dict_ids = part.group_key_dict_ids;      // (digits of nullable keys run to cardinality inclusive: the last one is NULL)
    part.group_key_dict_ids = nullptr;
    pg_result_free(&part);
    // numEntriesScannedPostFilter = numDocsScanned * projected columns of the WHOLE query (GroupByOperator.java:160-166): keys + inputs
    std::vector<int> projected;
    for (int g = 0; g < ng; ++g) if (std::find(projected.begin(), projected.end(), q->group_by_columns[g]) == projected.end()) projected.push_back(q->group_by_columns[g]);
    for (int a = 0; a < na; ++a) {
      const pg_aggregation& ag = q->aggregations[a];
      const bool reads = ag.function != PG_AGG_COUNT || ag.column >= 0;      // COUNT(col) keeps its input expression under null handling, nulls or not
      if (reads && ag.column >= 0 && std::find(projected.begin(), projected.end(), ag.column) == projected.end()) projected.push_back(ag.column);
    }
    out->stats.num_entries_scanned_post_filter = out->stats.num_docs_scanned * (int64_t)projected.size();
    for (int c : lane_cols) {
      FlatQuery lane;
      std::vector<FilterExpr> both;
      if (has_filter) both.push_back(filter_trues);
      both.push_back(NullRewriter::null_leaf(c, true));
      lane.emit(NullRewriter::combine(PG_FILTER_AND, std::move(both)));
      lane.finish(*q);
      lane.q.group_by_columns = keys.data();
      lane.q.num_groups_limit = kMaxGroupSlots;            // which groups exist is the base lane's decision: this lane reports all of its own
      std::vector<int> pos;
      for (int a = 0; a < na; ++a) if (q->aggregations[a].column == c) { lane.aggs.push_back(q->aggregations[a]); pos.push_back(a); }
      lane.q.aggregations = lane.aggs.data(); lane.q.num_aggregations = (int32_t)lane.aggs.size();
      memset(&part, 0, sizeof(part));
      st = execute_impl(seg, &lane.q, &part, nullptr, nullptr, 0, nullptr, false);
      if (st != PG_OK) { pg_result_free(&part); return st; }
      // both id lists ascend: one merge pass; lane groups the base lane did not admit (numGroupsLimit) are dropped
      int k = 0;
      for (int j = 0; j < part.num_groups; ++j) {
        while (k < num_groups && out->group_ids[k] < part.group_ids[j]) ++k;
        if (k == num_groups) break;
        if (out->group_ids[k] != part.group_ids[j]) continue;
        for (size_t i = 0; i < pos.size(); ++i) out->group_aggregations[(size_t)k * (size_t)na + (size_t)pos[i]] = part.group_aggregations[(size_t)j * (size_t)part.num_aggregations + i];
      }
      out->device_ms += part.device_ms;
      if (part.dominant_kernel_ms > out->dominant_kernel_ms) { out->dominant_kernel_ms = part.dominant_kernel_ms; out->dominant_kernel = part.dominant_kernel; }
      pg_result_free(&part);
    }
    return PG_OK;
  }
  if (lane_cols.empty()) return execute_impl(seg, &base.q, out, nullptr, nullptr, 0, nullptr);

  // Base lane: COUNT(*) and the aggregations of columns without nulls, over the filter itself.  It also yields numDocsScanned; the
  // metadata-only plan is off because the reference does not take it when any aggregated column has nulls (AggregationPlanNode.java:99-100).
  std::vector<int> base_pos;
  for (int a = 0; a < na; ++a) if (!rw.has_nulls(q->aggregations[a].column)) { base.aggs.push_back(q->aggregations[a]); base_pos.push_back(a); }
  const bool synthetic_count = base.aggs.empty();
  if (synthetic_count) base.aggs.push_back(pg_aggregation{PG_AGG_COUNT, -1});
  base.q.aggregations = base.aggs.data(); base.q.num_aggregations = (int32_t)base.aggs.size();
  pg_result part;
  memset(&part, 0, sizeof(part));
  st = execute_impl(seg, &base.q, &part, nullptr, nullptr, 0, nullptr, false);
  if (st != PG_OK) { pg_result_free(&part); return st; }
  memset(out, 0, sizeof(*out));
  out->num_aggregations = na;
  out->aggregations = (pg_agg_value*)calloc((size_t)std::max(na, 1), sizeof(pg_agg_value));
  out->stats = part.stats;
  out->device_ms = part.device_ms; out->dominant_kernel_ms = part.dominant_kernel_ms; out->dominant_kernel = part.dominant_kernel;
  if (!synthetic_count) for (size_t i = 0; i < base_pos.size(); ++i) out->aggregations[base_pos[i]] = part.aggregations[i];
  pg_result_free(&part);
  // numEntriesScannedPostFilter = numDocsScanned * projected columns of the WHOLE query (AggregationOperator.java:88-93)
  std::vector<int> projected;
  for (int a = 0; a < na; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    const bool reads = ag.function != PG_AGG_COUNT || ag.column >= 0;   // COUNT(col) keeps its input expression under null handling, nulls or not
    if (reads && ag.column >= 0 && std::find(projected.begin(), projected.end(), ag.column) == projected.end()) projected.push_back(ag.column);
  }
  out->stats.num_entries_scanned_post_filter = out->stats.num_docs_scanned * (int64_t)projected.size();

  for (int c : lane_cols) {
    FlatQuery lane;
    std::vector<FilterExpr> both;
    if (has_filter) both.push_back(filter_trues);
    both.push_back(NullRewriter::null_leaf(c, true));
    lane.emit(NullRewriter::combine(PG_FILTER_AND, std::move(both)));
    lane.finish(*q);
    std::vector<int> pos;
    for (int a = 0; a < na; ++a) if (q->aggregations[a].column == c) { lane.aggs.push_back(q->aggregations[a]); pos.push_back(a); }
    lane.q.aggregations = lane.aggs.data(); lane.q.num_aggregations = (int32_t)lane.aggs.size();
    memset(&part, 0, sizeof(part));
    st = execute_impl(seg, &lane.q, &part, nullptr, nullptr, 0, nullptr, false);
    if (st != PG_OK) { pg_result_free(&part); return st; }
    for (size_t i = 0; i < pos.size(); ++i) out->aggregations[pos[i]] = part.aggregations[i];
    out->device_ms += part.device_ms;
    if (part.dominant_kernel_ms > out->dominant_kernel_ms) { out->dominant_kernel_ms = part.dominant_kernel_ms; out->dominant_kernel = part.dominant_kernel; }
    pg_result_free(&part);
  }
  return PG_OK;
}

// numEntriesScannedInFilter of a filter that leap-frogs (pg_filter_stats.h, Plan::kReplay): every leaf's docId set comes off the device
// as a bitmap, the reference's iterator tree is replayed over them.  Sequential in the docId space, hence the segment-size limit.
static pg_status replay_filter_stats(pg_segment* seg, const pg_query* q, pg_result* out) {
  const size_t words = ((size_t)seg->num_docs + 63) / 64;
  std::vector<fstats::Words> leaf_words((size_t)q->num_predicates);
  for (int i = 0; i < q->num_filter_nodes; ++i) {
    const pg_filter_node& n = q->filter[i];
    if (n.op != PG_FILTER_LEAF || leaf_words[(size_t)n.predicate]) continue;
    const fstats::LeafClass c = fstats::classify(q->predicates[n.predicate]);
    if (c == fstats::LeafClass::kMatchAll || c == fstats::LeafClass::kEmpty) continue;
    auto w = std::make_shared<std::vector<uint64_t>>(std::max<size_t>(words, 1), 0ull);
    pg_filter_node leaf = n;
    pg_query lq;
    memset(&lq, 0, sizeof(lq));
    lq.filter = &leaf; lq.num_filter_nodes = 1;
    lq.predicates = q->predicates; lq.num_predicates = q->num_predicates;
    pg_status st = execute_impl(seg, &lq, nullptr, nullptr, w->data(), (int64_t)w->size(), nullptr);
    if (st != PG_OK) return st;
    leaf_words[(size_t)n.predicate] = std::move(w);
  }
  out->stats.num_entries_scanned_in_filter = fstats::replay(q, seg->num_docs, leaf_words);
  out->filter_entries_exact = 1;
  return PG_OK;
}

// The same count ON THE DEVICE, at any segment size, for the root ANDs pg_filter_fsm.h can compile (scan leaves, index-based leaves, ORs
// of leaves -- `a AND b AND c`, `a AND (b OR c)`, the reference's golden filter): every leaf's docId set stays on the device as a
// doc-order bitmap, the transducer's tables are built tile by tile and chained (pg_fsm_kernels.h).  Nothing but the count comes back.
// Layout of the pass's scratch (ExecCtx.d_fsm_scratch): L bitmaps of whole tiles | delta | tile tables | chunk tables | the count --
// and, for a machine with a NOT child (Fsm::marks: the episodes of pg_fsm_kernels.h), from the next 256-byte boundary on:
// episode count + final-pending flags | marks of every episode stream | chunk states | tile states | the tiles' unpaired closes | the tiles' last opens.
// A second walk of the docs behind the tile pass: the episodes of NOT children (one pass per episode stream), and -- round 6c -- the COUNT of
// machines of 9 .. 16 states over at most four inputs without episodes (one pass, no marks): their tile pass builds functions only
// (fsm_tile_fns_kernel) instead of walking sixteen chains of table reads per doc (fsm_tiles_kernel<16, L>).
static inline bool needs_second_walk(const fstats::Fsm& fsm) { return fsm.has_episodes() || (fsm.num_states > 8 && fsm.num_inputs <= 4); }
static inline int second_walk_passes(const fstats::Fsm& fsm) { return fsm.has_episodes() ? fsm.num_episode_streams() : 1; }
struct FsmScratch {
  size_t bitmap_bytes = 0, delta_bytes = 0, tables_bytes = 0, chunk_bytes = 0, total = 0;
  size_t episode_base = 0, chunk_state_bytes = 0, tile_state_bytes = 0, tile_pos_bytes = 0;
  size_t front_bytes = 0;            // machines with episodes: fsm_tile_fns_kernel's lane fronts (4 / 8 / 16 bytes a lane for <= 4 / 8 / 16 states), behind the last opens
  long long tiles = 0, chunks = 0;
  FsmScratch(const pg_segment* seg, const fstats::Fsm& fsm) {
    tiles = std::max<long long>(1, doc_tiles(seg));
    chunks = (tiles + kFsmChunk - 1) / kFsmChunk;
    bitmap_bytes = (size_t)tiles * 256;
    delta_bytes = (((size_t)fsm.num_states << fsm.num_inputs) + 255) & ~(size_t)255;
    tables_bytes = (size_t)tiles * (size_t)fsm.num_states * 4;
    chunk_bytes = ((size_t)chunks * (size_t)fsm.num_states * 4 + 255) & ~(size_t)255;
    total = bitmap_bytes * (size_t)fsm.num_inputs + delta_bytes + tables_bytes + chunk_bytes + 256;
    if (needs_second_walk(fsm)) {
      episode_base = (total + 255) & ~(size_t)255;
      chunk_state_bytes = ((size_t)chunks + 255) & ~(size_t)255;
      tile_state_bytes = ((size_t)tiles + 255) & ~(size_t)255;
      tile_pos_bytes = ((size_t)tiles * 4 + 255) & ~(size_t)255;
      total = episode_base + 256 + delta_bytes * (size_t)second_walk_passes(fsm) + chunk_state_bytes + tile_state_bytes + 2 * tile_pos_bytes;
      front_bytes = (size_t)tiles * 64 * (fsm.num_states <= 4 ? 4 : (fsm.num_states <= 8 ? 8 : 16));
      total += front_bytes;
    }
  }
};
// The context's scratch, grown when needed, and where every input's bitmap goes.  (execute_impl, with the context it runs on.)
static pg_status prepare_fsm_side(pg_segment* seg, ExecCtx* ctx, const fstats::Fsm& fsm, FsmSide* side) {
  const FsmScratch lay(seg, fsm);
  // fsm_finish_kernel keeps one table per chunk in LDS (chunks * S * 4 bytes): 16 states near 2^31 docs pass 64 KB -- such a machine is not counted here
  if ((size_t)lay.chunks * (size_t)fsm.num_states * 4 > (60u << 10)) return fail(PG_ERR_UNSUPPORTED, "transducer pass: %lld chunks x %d states exceed the finish kernel's LDS", lay.chunks, fsm.num_states);
  if (ctx->fsm_scratch_bytes < lay.total) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->d_fsm_scratch) (void)hipFree(ctx->d_fsm_scratch);
    seg->device_bytes -= ctx->fsm_scratch_bytes;               // (the scratch is part of what pg_segment_device_bytes reports: the HBM budget of the caller sees it)
    ctx->d_fsm_scratch = nullptr; ctx->fsm_scratch_bytes = 0;
    HIP_TRY(hipMalloc((void**)&ctx->d_fsm_scratch, lay.total));
    ctx->fsm_scratch_bytes = lay.total;
    seg->device_bytes += lay.total;
  }
  if (!ctx->h_fsm_stage) HIP_TRY(hipHostMalloc((void**)&ctx->h_fsm_stage, kFsmStageBytes, hipHostMallocDefault));
  for (hipEvent_t& e : ctx->ev_pass) if (!e) HIP_TRY(hipEventCreate(&e));
  const fstats::Fsm* keep = side->fsm;
  *side = FsmSide();
  side->fsm = keep ? keep : &fsm;
  for (int i = 0; i < fsm.num_inputs; ++i) side->bitmap[i] = reinterpret_cast<uint32_t*>(ctx->d_fsm_scratch + lay.bitmap_bytes * (size_t)i);
  uint8_t* at = ctx->d_fsm_scratch + lay.bitmap_bytes * (size_t)fsm.num_inputs + lay.delta_bytes;
  side->tables = reinterpret_cast<uint32_t*>(at); at += lay.tables_bytes;
  side->chunks = reinterpret_cast<uint32_t*>(at); at += lay.chunk_bytes;
  side->entries = reinterpret_cast<unsigned long long*>(at);
  side->num_tiles = lay.tiles; side->num_chunks = lay.chunks;
  side->prepared = true;
  return PG_OK;
}

// Behind the query's own kernels, on the query's stream, with the context still held: kernels and copies are enqueued, ONE synchronisation
// at the end (rounds 4-5: the NULL stream, four synchronous copies, under a segment-wide mutex).  For timed runs the pass is bracketed by
// ctx->ev_pass and added to device_ms by the caller.
static pg_status device_fsm_filter_stats(pg_segment* seg, ExecCtx* ctx, const pg_query* q, const FsmSide& side, pg_result* out) {
  const fstats::Fsm& fsm = *side.fsm;
  hipStream_t stream = ctx->stream;
  const FsmScratch lay(seg, fsm);
  const long long tiles = lay.tiles, chunks = lay.chunks;
  const int L = fsm.num_inputs, S = fsm.num_states;
  static const bool trace = getenv("PINOT_GPU_FSM_TRACE") != nullptr;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
  const auto t_begin = now();
  uint8_t* d_base = ctx->d_fsm_scratch;
  if ((((size_t)fsm.num_states << fsm.num_inputs) * (size_t)(1 + second_walk_passes(fsm)) + 64) > kFsmStageBytes) return fail(PG_ERR_INTERNAL, "transducer tables exceed the pinned staging area");
  FsmParams fp;
  memset(&fp, 0, sizeof(fp));
  int scanned_again = 0;
  for (int i = 0; i < L; ++i) {
    fp.leaf[i] = side.bitmap[i];
    if (side.kernel_wrote && side.mapped[i]) continue;        // the query's own kernel left it behind
    // a leaf the kernel did not evaluate as a node of its own (the inverted-index children of the root AND are one merged leaf there),
    // or a kernel without the store: this leaf's docId set by a pass of its own
    ++scanned_again;
    HIP_TRY(hipMemset(reinterpret_cast<uint8_t*>(side.bitmap[i]) + (lay.bitmap_bytes - 256), 0, 256));      // the last tile's dwords past numDocs
    pg_filter_node leaf;
    memset(&leaf, 0, sizeof(leaf));
    leaf.op = PG_FILTER_LEAF; leaf.predicate = fsm.input_predicate[(size_t)i];
    pg_query lq;
    memset(&lq, 0, sizeof(lq));
    lq.filter = &leaf; lq.num_filter_nodes = 1;
    lq.predicates = q->predicates; lq.num_predicates = q->num_predicates;
    const pg_status st = execute_impl(seg, &lq, nullptr, reinterpret_cast<unsigned long long*>(side.bitmap[i]), nullptr, 0, nullptr);      // (returns with the copy done)
    if (st != PG_OK) return st;
  }
  const auto t_leaves = now();
  const bool timed_pass = (g_engine.flags & PG_CFG_TIME_KERNELS) != 0;
  if (timed_pass) HIP_TRY(hipEventRecord(ctx->ev_pass[0], stream));
  uint8_t* at = d_base + lay.bitmap_bytes * (size_t)L;
  uint8_t* d_delta = at; at += lay.delta_bytes;
  uint32_t* d_tables = reinterpret_cast<uint32_t*>(at); at += lay.tables_bytes;
  uint32_t* d_chunks = reinterpret_cast<uint32_t*>(at); at += lay.chunk_bytes;
  unsigned long long* d_entries = reinterpret_cast<unsigned long long*>(at);
  uint8_t* const h_delta = ctx->h_fsm_stage + 64;
  uint8_t* const h_marks = h_delta + ((size_t)S << L);
  memcpy(h_delta, fsm.delta.data(), (size_t)S << L);
  HIP_TRY(hipMemcpyAsync(d_delta, h_delta, (size_t)S << L, hipMemcpyHostToDevice, stream));
  fp.delta = d_delta; fp.tables = d_tables;
  fp.num_inputs = L; fp.num_states = S; fp.num_docs = seg->num_docs; fp.num_tiles = (int32_t)tiles;
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((tiles + 3) / 4, (long long)seg->num_cus * 8));
#define PG_FSM_LAUNCH(SM, LM) fsm_tiles_kernel<SM, LM><<<dim3(blocks), dim3(256), 0, stream>>>(fp)
// (a machine over two inputs has at most three states -- 350 000 random root ANDs over two predicates, tools/kernel_coverage.py's search:
//  the <8, 2>, <16, 2> table walks and the eight-state byte-function walk over two inputs were instantiations no query could reach;
//  the coverage gate of round 5 found them, they are gone: such a machine, should one ever exist, walks the three-input form)
#define PG_FSM_LAUNCH_L(SM) do { if (L <= 2 && SM <= 4) PG_FSM_LAUNCH((SM <= 4 ? SM : 4), 2); else if (L <= 3) PG_FSM_LAUNCH(SM, 3); else if (L <= 4) PG_FSM_LAUNCH(SM, 4); else if (L <= 6) PG_FSM_LAUNCH(SM, 6); else PG_FSM_LAUNCH(SM, 8); } while (0)
  const bool perm_walk = g_engine.fsm_perm;
  // (the byte-function walk keeps a lane's entries per entry state in ONE byte: 16 steps x two docs x at most 7 entries per doc.  A doc
  //  costs more than 7 only when the tree names the same predicate in many leaves -- such machines walk tables)
  int max_inc = 0;
  for (uint8_t d : fsm.delta) max_inc = std::max(max_inc, (int)(d >> 4));
  // (machines with episodes over at most four inputs: the tile pass builds the tiles' functions only and leaves every lane's front; the range
  //  kernel of the first episode stream counts the per-doc entries -- see fsm_tile_fns_kernel)
  // (count_pass: nine to sixteen states WITHOUT episodes -- the same two kernels, the range kernel as the counter: one pass with no marks)
  const bool count_pass = perm_walk && !fsm.has_episodes() && S > 8 && S <= 16 && L <= 4;
  const bool fns_pass = perm_walk && S <= 16 && L <= 4 && (fsm.has_episodes() || count_pass);
  if (fns_pass) {
    fp.lane_front = reinterpret_cast<uint32_t*>(d_base + lay.episode_base + 256 + lay.delta_bytes * (size_t)second_walk_passes(fsm) + lay.chunk_state_bytes + lay.tile_state_bytes + 2 * lay.tile_pos_bytes);
    if (S <= 4) { if (L <= 2) fsm_tile_fns_kernel<4, 2><<<dim3(blocks), dim3(256), 0, stream>>>(fp); else fsm_tile_fns_kernel<4, 4><<<dim3(blocks), dim3(256), 0, stream>>>(fp); }
    else if (S <= 8) { if (L <= 2) fsm_tile_fns_kernel<8, 2><<<dim3(blocks), dim3(256), 0, stream>>>(fp); else fsm_tile_fns_kernel<8, 4><<<dim3(blocks), dim3(256), 0, stream>>>(fp); }
    else if (L <= 3) fsm_tile_fns_kernel<16, 3><<<dim3(blocks), dim3(256), 0, stream>>>(fp);
    else fsm_tile_fns_kernel<16, 4><<<dim3(blocks), dim3(256), 0, stream>>>(fp);
  }
  else if (S <= 4 && L <= 4 && max_inc <= 7 && perm_walk) {
    if (L <= 2) fsm_tiles_perm_kernel<2><<<dim3(blocks), dim3(256), 0, stream>>>(fp);
    else if (L <= 3) fsm_tiles_perm_kernel<3><<<dim3(blocks), dim3(256), 0, stream>>>(fp);
    else fsm_tiles_perm_kernel<4><<<dim3(blocks), dim3(256), 0, stream>>>(fp);
  }
  else if (S <= 8 && L <= 4 && max_inc <= 7 && perm_walk) {
    if (L <= 3) fsm_tiles_perm8_kernel<3><<<dim3(blocks), dim3(256), 0, stream>>>(fp);
    else fsm_tiles_perm8_kernel<4><<<dim3(blocks), dim3(256), 0, stream>>>(fp);
  }
  else if (S <= 2) PG_FSM_LAUNCH_L(2);
  else if (S <= 4) PG_FSM_LAUNCH_L(4);
  else if (S <= 8) PG_FSM_LAUNCH_L(8);
  else PG_FSM_LAUNCH_L(16);
#undef PG_FSM_LAUNCH_L
#undef PG_FSM_LAUNCH
  HIP_TRY(hipGetLastError());
  if (trace) HIP_TRY(hipDeviceSynchronize());
  const auto t_tiles = now();
  fsm_chain_kernel<<<dim3((unsigned)chunks), dim3(1024), 0, stream>>>(d_tables, tiles, S, d_chunks);
  HIP_TRY(hipGetLastError());
  fsm_finish_kernel<<<dim3(1), dim3(1024), (size_t)chunks * (size_t)S * 4, stream>>>(d_chunks, (int)chunks, S, d_entries);
  HIP_TRY(hipGetLastError());
  unsigned long long entries = 0, episodes = 0;
  if (fsm.has_episodes() || count_pass) {
    // A NOT child over a scan leaf: what its leaf scans in 256-doc batches is charged per episode (pg_fsm_kernels.h "NOT children").  The
    // tables of the count, walked downwards, give every tile its entry state; a second walk of the docs pairs the opens and the closes.
    // (count_pass: no episodes -- one such walk with all-zero marks, for the per-doc entries alone)
    uint8_t* eb = d_base + lay.episode_base;
    unsigned long long* d_episodes = reinterpret_cast<unsigned long long*>(eb);
    const int streams = second_walk_passes(fsm);
    uint8_t* d_marks_base = eb + 256;
    uint8_t* d_chunk_state = d_marks_base + lay.delta_bytes * (size_t)streams;
    uint8_t* d_tile_state = d_chunk_state + lay.chunk_state_bytes;
    int32_t* d_first_close = reinterpret_cast<int32_t*>(d_tile_state + lay.tile_state_bytes);
    int32_t* d_last_open = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(d_first_close) + lay.tile_pos_bytes);
    HIP_TRY(hipMemsetAsync(eb, 0, 64, stream));
    fsm_chunk_states_kernel<<<dim3(1), dim3(1024), (size_t)chunks * (size_t)S * 4, stream>>>(d_chunks, (int)chunks, S, d_chunk_state);
    HIP_TRY(hipGetLastError());
    fsm_tile_states_kernel<<<dim3((unsigned)chunks), dim3(1024), 0, stream>>>(d_tables, tiles, S, d_chunk_state, d_tile_state);
    HIP_TRY(hipGetLastError());
    // every NOT child over a scan leaf has an episode stream of its own: the same machine and entry states, its own marks, its own
    // final-pending flag; the streams' entries add up in *d_episodes (the kernels add into it)
    for (int k = 0; k < streams; ++k) {
    uint8_t* const d_marks = d_marks_base + lay.delta_bytes * (size_t)k;
    uint8_t* const h_marks_k = h_marks + ((size_t)S << L) * (size_t)k;
    int32_t* const d_final_pending = reinterpret_cast<int32_t*>(eb + 8) + k;
    const uint32_t pending_states = count_pass ? 0u : fsm.stream_pending(k);
    if (count_pass) memset(h_marks_k, 0, (size_t)S << L);
    else memcpy(h_marks_k, fsm.stream_marks(k).data(), (size_t)S << L);
    HIP_TRY(hipMemcpyAsync(d_marks, h_marks_k, (size_t)S << L, hipMemcpyHostToDevice, stream));
    if (fns_pass) {
      // machines of at most sixteen states over at most four inputs: the tile pass (fsm_tile_fns_kernel) left every lane's front; one chain per
      // lane from the real entry state, a contiguous range of tiles per wavefront -- one record per RANGE for the finish kernel
      // (pg_fsm_kernels.h "Round 6", "Round 6c")
      const long long num_ranges = std::min<long long>(tiles, (long long)blocks * 4);
      FsmEpisodeRangeParams rp;
      memset(&rp, 0, sizeof(rp));
      for (int i = 0; i < L; ++i) rp.leaf[i] = fp.leaf[i];
      rp.delta = d_delta; rp.marks = d_marks; rp.tile_state = d_tile_state;
      rp.range_first_close = d_first_close; rp.range_last_open = d_last_open;
      rp.episode_entries = d_episodes; rp.final_pending = d_final_pending;
      rp.pending_states = pending_states;
      rp.num_inputs = L; rp.num_states = S; rp.num_docs = seg->num_docs; rp.num_tiles = (int32_t)tiles; rp.num_ranges = (int32_t)num_ranges;
      rp.count_entries = k == 0 ? 1 : 0;      // (the tile pass built functions only: the first stream's walk counts what the docs cost)
      rp.lane_front = fp.lane_front;
      const dim3 rgrid((unsigned)((num_ranges + 3) / 4));
      if (S > 8) fsm_episode_ranges_kernel<16, 4><<<rgrid, dim3(256), 0, stream>>>(rp);
      else if (S <= 4) { if (L <= 2) fsm_episode_ranges_kernel<4, 2><<<rgrid, dim3(256), 0, stream>>>(rp); else fsm_episode_ranges_kernel<4, 4><<<rgrid, dim3(256), 0, stream>>>(rp); }
      else { if (L <= 2) fsm_episode_ranges_kernel<8, 2><<<rgrid, dim3(256), 0, stream>>>(rp); else fsm_episode_ranges_kernel<8, 4><<<rgrid, dim3(256), 0, stream>>>(rp); }
      HIP_TRY(hipGetLastError());
      fsm_episode_finish_kernel<<<dim3(1), dim3(1024), 0, stream>>>(d_first_close, d_last_open, (int)num_ranges, seg->num_docs, d_final_pending, d_episodes);
      HIP_TRY(hipGetLastError());
    } else {
      FsmEpisodeParams ep;
      memset(&ep, 0, sizeof(ep));
      for (int i = 0; i < L; ++i) ep.leaf[i] = fp.leaf[i];
      ep.delta = d_delta; ep.marks = d_marks; ep.tile_state = d_tile_state;
      ep.tile_first_close = d_first_close; ep.tile_last_open = d_last_open;
      ep.episode_entries = d_episodes; ep.final_pending = d_final_pending;
      ep.pending_states = pending_states;
      ep.num_inputs = L; ep.num_states = S; ep.num_docs = seg->num_docs; ep.num_tiles = (int32_t)tiles;
      fsm_episode_tiles_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(ep);
      HIP_TRY(hipGetLastError());
      fsm_episode_finish_kernel<<<dim3(1), dim3(1024), 0, stream>>>(d_first_close, d_last_open, (int)tiles, seg->num_docs, d_final_pending, d_episodes);
      HIP_TRY(hipGetLastError());
    }
    }
    HIP_TRY(hipMemcpyAsync(ctx->h_fsm_stage + 8, d_episodes, 8, hipMemcpyDeviceToHost, stream));
  }
  HIP_TRY(hipMemcpyAsync(ctx->h_fsm_stage, d_entries, 8, hipMemcpyDeviceToHost, stream));
  if (timed_pass) HIP_TRY(hipEventRecord(ctx->ev_pass[1], stream));
  HIP_TRY(hipStreamSynchronize(stream));
  memcpy(&entries, ctx->h_fsm_stage, 8);
  if (fsm.has_episodes() || count_pass) memcpy(&episodes, ctx->h_fsm_stage + 8, 8);
  entries += episodes;
  if (timed_pass) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_pass[0], ctx->ev_pass[1]));
    out->device_ms += ms;
  }
  if (trace) fprintf(stderr, "fsm stats: %d inputs %d states %lld tiles: %d leaf bitmaps scanned again %.1f us, tables kernel %.1f us, chain+finish+copy %.1f us%s\n", L, S, tiles,
                     scanned_again, us(t_begin, t_leaves), us(t_leaves, t_tiles), us(t_tiles, now()), fsm.has_episodes() ? " (with the episodes of a NOT child)" : "");
  out->stats.num_entries_scanned_in_filter = (int64_t)entries;
  out->filter_entries_exact = 1;
  return PG_OK;
}

// pg_execute, or -- with `defer` -- its first half: kDeferred means the query was lowered but not launched (see Deferred).
static pg_status execute_one(pg_segment* segment, const pg_query* query, pg_result* out_result, Deferred* defer) {
  if (!out_result) return fail(PG_ERR_INVALID_ARGUMENT, "null result");
  memset(out_result, 0, sizeof(*out_result));     // before anything can fail: every error path below ends in pg_result_free(out_result)
  const bool null_handling = query && (query->flags & PG_QUERY_NULL_HANDLING);
  // A leap-frogging filter whose shape compiles into the transducer of pg_filter_fsm.h is counted on the device at any size
  // (PINOT_GPU_FSM_STATS=0: never): the query's own kernel leaves the leaves' bitmaps in the segment's scratch (one such query at a
  // time per segment), the pass follows.  Other shapes: the host's replay of the iterator tree up to
  // PINOT_GPU_EXACT_FILTER_STATS_DOCS docs, else the upper bound stands.
  const bool bound_ok = query && (query->flags & PG_QUERY_STATS_UPPER_BOUND_OK);      // the caller takes the upper bound: no pass, no replay
  const bool use_fsm = g_engine.fsm_stats && !bound_ok;
  fstats::Fsm fsm;
  FsmSide side;
  if (use_fsm && !null_handling && segment && query && query->num_filter_nodes >= 3 && query->filter && query->predicates) {
    int scan_leaves = 0;
    // (the machine only: execute_impl gives it the scratch of the context the query runs on and runs the pass behind the query's kernels, on
    //  their stream -- two such queries on one segment overlap like any others; rounds 4-5 held a segment-wide mutex across query and pass)
    if (fstats::choose_plan(query, &scan_leaves) == fstats::Plan::kReplay && fstats::compile_fsm(query, &fsm) && (g_engine.fsm_episodes || !fsm.has_episodes())) side.fsm = &fsm;
  }
  pg_status st = null_handling ? execute_null_handling(segment, query, out_result, nullptr, 0, nullptr)
                               : execute_impl(segment, query, out_result, nullptr, nullptr, 0, nullptr, true, defer, side.fsm != nullptr ? &side : nullptr);
  if (st == kDeferred) return st;
  // (enableNullHandling changes the iterator tree -- nulls are or-ed in, NOT takes the falses: the upper bound stands there)
  if (st == PG_OK && !null_handling && !bound_ok && !out_result->filter_entries_exact && (int64_t)segment->num_docs <= g_engine.exact_stats_docs)
    st = replay_filter_stats(segment, query, out_result);
  if (st != PG_OK) pg_result_free(out_result);
  return st;
}

// ---- PG_AGG_DISTINCTCOUNT: the dictId bitsets of dictionary columns (pg_scan_distinct.h) ----
// A query with a DISTINCTCOUNT is answered in up to two runs over the same filter, on the same stream one after the other:
//   the ordinary query  -- the caller's aggregation list with every DISTINCTCOUNT turned into COUNT(*): every other function, the
//                          statistics and (GROUP BY) the list of groups that exist come from the paths they take today, untouched;
//   the bitset pass     -- the same list with everything BUT the DISTINCTCOUNTs turned into COUNT(*), flagged kQueryDistinctPass: one launch
//                          of scan_distinct_kernel / group_distinct_kernel behind the same lowered filter.
// `DISTINCTCOUNT(c1..c4) [, COUNT(*)]` without GROUP BY is the pass alone: its kernel counts the docs and the filter entries itself.
// No filter (or one that matches everything), no GROUP BY, every function answerable from metadata: nothing is launched, every bit below the
// cardinality is set (AggregationPlanNode.java:50-54,170-173; NonScanBasedAggregationOperator.java:106-112).
// pg_query.flags bits above the public ones are the library's own (execute_null_handling / execute_distinct -> execute_impl): a caller that sets
// one is refused at every entry point that takes a query.
constexpr int32_t kQueryPublicFlags = PG_QUERY_NULL_HANDLING | PG_QUERY_STATS_UPPER_BOUND_OK;
static bool reserved_flags(const pg_query* q) { return q != nullptr && (q->flags & ~kQueryPublicFlags) != 0; }
static pg_status fail_reserved_flags(const pg_query* q) { return fail(PG_ERR_INVALID_ARGUMENT, "pg_query.flags 0x%x sets reserved bits", (unsigned)q->flags); }
static bool has_distinct(const pg_query* q) {      // (a DISTINCTCOUNTHLL is planned and executed with the DISTINCTCOUNTs: plan_distinct / execute_distinct)
  if (!q || !q->aggregations) return false;
  for (int a = 0; a < q->num_aggregations; ++a) if (q->aggregations[a].function == PG_AGG_DISTINCTCOUNT || is_hll_function(q->aggregations[a].function)) return true;
  return false;
}
// The function words of a query: bits above the low byte belong to PG_AGG_HLL(log2m) alone, and its log2m lies in [PG_HLL_MIN_LOG2M, PG_HLL_MAX_LOG2M].
static const pg_aggregation* bad_function_word(const pg_query* q) {
  if (!q || !q->aggregations) return nullptr;
  for (int a = 0; a < q->num_aggregations; ++a) {
    const int32_t f = q->aggregations[a].function;
    if ((f & ~0xFF) == 0) continue;
    if (!is_hll_function(f) || (f >> 8) < PG_HLL_MIN_LOG2M || (f >> 8) > PG_HLL_MAX_LOG2M) return &q->aggregations[a];
  }
  return nullptr;
}
static pg_status fail_function_word(const pg_aggregation* ag) {
  if (is_hll_function(ag->function)) return fail(PG_ERR_INVALID_ARGUMENT, "DISTINCTCOUNTHLL with log2m %d: outside [%d, %d]", (int)(ag->function >> 8), PG_HLL_MIN_LOG2M, PG_HLL_MAX_LOG2M);
  return fail(PG_ERR_INVALID_ARGUMENT, "aggregation function word 0x%x sets bits above the function's byte", (unsigned)ag->function);
}
static pg_status check_ordinary_query(const pg_segment* segment, const pg_query* query);
// ---- PG_AGG_PERCENTILE / PG_AGG_DISTINCTCOUNT on raw columns: the collect pass (pg_scan_collect.h) ----
// A raw (no-dictionary) column has no dictId to count or to set a bit for: the pass writes the order image of every matching doc's value into a
// list per column, sorts it and run-length encodes it (arm_collect / harvest_collect); the runs are pg_result_value_counts' answer.  The query runs exactly as
// the dictionary forms do -- the ordinary query, then the pass behind the same filter, or the pass alone -- with kQueryCollectPass set beside the
// pass's own flag.  A query's PERCENTILE / DISTINCTCOUNT columns are all raw or all dictionary-encoded.
// The plan-time bound of the lists: every doc could match (pg_query_check knows no better, and pg_execute must agree with it).
static pg_status plan_collect_bytes(const pg_segment* seg, const char* function, size_t columns, bool grouped) {
  const unsigned long long bytes = (unsigned long long)std::max<int64_t>(seg->num_docs, 0) * (16ull * (unsigned long long)columns + (grouped ? 8ull : 0ull));
  if (bytes > PG_COLLECT_MAX_BYTES)
    return fail(PG_ERR_UNSUPPORTED, "%s value lists of %llu bytes over raw columns exceed PG_COLLECT_MAX_BYTES (%llu) -- CPU plan", function, bytes, (unsigned long long)PG_COLLECT_MAX_BYTES);
  if (bytes > g_engine.group_table_bytes)
    return fail(PG_ERR_UNSUPPORTED, "%s value lists of %llu bytes over raw columns exceed the %llu-byte budget (PINOT_GPU_GROUP_TABLE_BYTES)", function, bytes, (unsigned long long)g_engine.group_table_bytes);
  return PG_OK;
}
// A raw column the pass can read: fixed-width numeric values.  (pg_segment_open keeps nothing else resident -- STRING and BYTES columns are
// refused there, LZ4 / SNAPPY chunks are decoded there -- so this is a safety net behind it.)
static pg_status plan_collect_column(const ColumnDev& col, const char* function) {
  // The pass is opt-in (PINOT_GPU_COLLECT=1): a deployment that has not asked for it sees the decline it has always seen, and its plans do not change
  // under it -- the lists cost up to 16 bytes of HBM per doc and column for the length of a query, which the dictionary forms never did.
  if (!g_engine.collect)
    return fail(PG_ERR_UNSUPPORTED, "%s on raw (no-dictionary) column %s: the collect pass is off (PINOT_GPU_COLLECT=1 turns it on) -- CPU plan", function, col.name.c_str());
  if (col.encoding != PG_FWD_RAW_FIXED_BYTE || col.stored_type < PG_TYPE_INT || col.stored_type > PG_TYPE_DOUBLE || col.d_fwd == nullptr)
    return fail(PG_ERR_UNSUPPORTED, "%s on column %s: neither dictionary-encoded nor raw fixed-width INT / LONG / FLOAT / DOUBLE -- CPU plan", function, col.name.c_str());
  return PG_OK;
}
// The pass's lists -> the result's.  Aggregation only: they are final.  GROUP BY: the runs of all raw group ids, cut into the rows of the groups the
// ordinary query reports (group_ids: ascending raw ids, key kind 0); a row's count is its list's length (PERCENTILE) or its runs (DISTINCTCOUNT).
static pg_status finish_value_lists(const pg_query* q, pg_result* out, ResultInternal* got, int function) {
  const int na = q->num_aggregations;
  if (q->num_group_by == 0) return PG_OK;
  const int num_groups = out->num_groups;
  for (ValueList& m : got->values) {
    if (!m.grouped_in_transit) return fail(PG_ERR_INTERNAL, "a value list without group ids under GROUP BY");
    ValueList cut;
    cut.aggregation = m.aggregation; cut.rows = num_groups;
    cut.offsets.reserve((size_t)num_groups + 1);
    cut.offsets.push_back(0);
    const size_t num_runs = m.value_bits.size();
    size_t r = 0;
    for (int k = 0; k < num_groups; ++k) {
      const uint32_t row = (uint32_t)out->group_ids[k];
      if (r < num_runs && m.run_rows[r] < row) return fail(PG_ERR_INTERNAL, "values of raw group id %u, which the ordinary query does not report", m.run_rows[r]);
      int64_t docs = 0, runs = 0;
      for (; r < num_runs && m.run_rows[r] == row; ++r, ++runs) docs += m.counts[r];
      cut.offsets.push_back(r);
      pg_agg_value* v = &out->group_aggregations[(size_t)k * (size_t)na + (size_t)m.aggregation];
      memset(v, 0, sizeof(*v));
      empty_agg_value(v, function == PG_AGG_PERCENTILE ? docs : runs);
    }
    if (r != num_runs) return fail(PG_ERR_INTERNAL, "values of raw group id %u, which the ordinary query does not report", m.run_rows[r]);
    // (the runs are already in the rows' order: only the offsets are new)
    cut.value_bits = std::move(m.value_bits); cut.counts = std::move(m.counts);
    m = std::move(cut);
  }
  return PG_OK;
}
// ---- what plan_distinct / plan_percentile and execute_distinct / execute_percentile share (`who`: the function's name in the messages) ----
struct PassPlan {
  std::vector<pg_aggregation> base_aggs, pass_aggs;
  pg_query base, pass;               // the ordinary query; the pass
  bool pass_alone = false;           // FUNCTION(..) [, COUNT(*)] without GROUP BY: one launch
  int num_projected = 0;             // distinct columns the whole query projects (numEntriesScannedPostFilter = numDocsScanned x this)
};
// The pass kernels evaluate the lane-private filter: range leaves on raw 8-byte / FLOAT columns are not in it.  match_all: the filter is absent or
// matches every doc; filter_stages_set: a dictId-set leaf (an IN list) wants its staged area in LDS.
static pg_status plan_pass_filter(const pg_segment* seg, const pg_query* q, const char* who, bool* match_all, bool* filter_stages_set) {
  *match_all = q->num_filter_nodes == 0; *filter_stages_set = false;
  for (int n = 0; n < q->num_filter_nodes; ++n) {
    if (q->filter[n].op != PG_FILTER_LEAF) continue;
    if (q->filter[n].predicate < 0 || q->filter[n].predicate >= q->num_predicates) return fail(PG_ERR_INVALID_ARGUMENT, "filter node %d: bad predicate index", n);
    const pg_predicate& pr = q->predicates[q->filter[n].predicate];
    if (pr.kind == PG_PRED_RAW_RANGE && pr.column >= 0 && pr.column < (int)seg->cols.size() && seg->cols[(size_t)pr.column].stored_type != PG_TYPE_INT)
      return fail(PG_ERR_UNSUPPORTED, "%s beside a range predicate on raw LONG / FLOAT / DOUBLE column %s -- CPU plan", who, seg->cols[(size_t)pr.column].name.c_str());
    if (pr.kind == PG_PRED_DICT_SET) *filter_stages_set = true;
    if (q->num_filter_nodes == 1) *match_all = (pr.kind == PG_PRED_MATCH_ALL && !pr.exclusive) || (pr.kind == PG_PRED_MATCH_NONE && pr.exclusive);
  }
  return PG_OK;
}
// GROUP BY of a pass query: an int key space that numGroupsLimit can never cut, keys the kernel decodes as dictIds (dictionary columns, raw
// columns through their offset key images).  Projects the key columns; *product: the raw group ids, the rows of the pass's matrices.
static pg_status plan_pass_keys(const pg_segment* seg, const pg_query* q, const char* who, std::vector<int>* projected, unsigned long long* product) {
  const int ng = q->num_group_by, num_cols_total = (int)seg->cols.size();
  const bool null_handling = (q->flags & PG_QUERY_NULL_HANDLING) != 0;
  if (ng > kMaxDistinctKeys) return fail(PG_ERR_UNSUPPORTED, "%s with more than %d group-by columns -- CPU plan", who, kMaxDistinctKeys);
  std::vector<int> cards;
  for (int g = 0; g < ng; ++g) {
    int c = q->group_by_columns[g];
    if (c < 0 || c >= num_cols_total) return fail(PG_ERR_INVALID_ARGUMENT, "group-by column %d out of range", c);
    if (std::find(projected->begin(), projected->end(), c) == projected->end()) projected->push_back(c);
    if (null_handling && seg->cols[(size_t)c].d_null_bitmap != nullptr)
      return fail(PG_ERR_UNSUPPORTED, "%s grouped by nullable column %s under null handling -- CPU plan", who, seg->cols[(size_t)c].name.c_str());
    if (seg->cols[(size_t)c].encoding != PG_FWD_FIXED_BIT_DICT) {
      const int image = seg->cols[(size_t)c].keyimage_column;
      if (image < 0 || seg->cols[(size_t)image].rank_image)
        return fail(PG_ERR_UNSUPPORTED, "%s grouped by raw column %s, which is not keyed by offset -- CPU plan", who, seg->cols[(size_t)c].name.c_str());
      c = image;
    }
    cards.push_back(seg->cols[(size_t)c].cardinality);
  }
  HashPlan hash_plan;
  const pg_status hst = plan_hash_holder(seg, cards, &hash_plan); if (hst != PG_OK) return hst;
  if (hash_plan.kind != 0) return fail(PG_ERR_UNSUPPORTED, "%s grouped over a key space of kind %d (raw keys beyond an int: the hashed holders) -- CPU plan", who, hash_plan.kind);
  *product = 1;
  for (int card : cards) *product *= (unsigned long long)std::max(card, 1);
  const long long limit = groups_limit(q);
  if (*product > (unsigned long long)limit)
    return fail(PG_ERR_UNSUPPORTED, "%s grouped over %llu raw keys, above numGroupsLimit %lld (the limit could bind) -- CPU plan", who, *product, limit);
  return PG_OK;
}
// The two queries that answer the caller's: the ordinary query -- every aggregation of the pass (is_pass) turned into COUNT(*) -- and the pass, with
// everything BUT those turned into COUNT(*) and pass_flags set.  Ends with the plan-time checks of both (check_pass false: only the ordinary one runs).
// base_function: what a pass aggregation becomes in the ordinary query -- COUNT(*), or that function on the same column (VARIANCE: AVG).
static pg_status split_pass_query(const pg_segment* seg, const pg_query* q, PassPlan* plan, bool (*is_pass)(int32_t function), int32_t pass_flags, bool check_pass = true,
                                  int32_t base_function = PG_AGG_COUNT) {
  const int na = q->num_aggregations;
  plan->base_aggs.assign(q->aggregations, q->aggregations + na);
  plan->pass_aggs.assign(q->aggregations, q->aggregations + na);
  for (int a = 0; a < na; ++a) {
    if (!is_pass(q->aggregations[a].function)) plan->pass_aggs[(size_t)a] = pg_aggregation{PG_AGG_COUNT, -1};
    else plan->base_aggs[(size_t)a] = base_function == PG_AGG_COUNT ? pg_aggregation{PG_AGG_COUNT, -1} : pg_aggregation{base_function, q->aggregations[a].column};
  }
  plan->base = *q; plan->base.aggregations = plan->base_aggs.data();
  plan->pass = *q; plan->pass.aggregations = plan->pass_aggs.data();
  plan->pass.flags |= pass_flags;
  if (!plan->pass_alone) plan->pass.flags |= PG_QUERY_STATS_UPPER_BOUND_OK;      // (the ordinary query brings the statistics)
  pg_status st = plan->pass_alone ? PG_OK : check_ordinary_query(seg, &plan->base);
  if (st == PG_OK && check_pass) st = check_ordinary_query(seg, &plan->pass);
  return st;
}
// The ordinary query into `out` and the pass behind it on the same stream into `pass` -- or the pass alone into `out`.  The pass's device time joins
// the result's, its sets come back in *got (null: it left none); the caller frees `pass`.  A failure of the pass leaves `out` released and zeroed.
static pg_status execute_base_and_pass(pg_segment* seg, const PassPlan& plan, pg_result* out, pg_result* pass, std::unique_ptr<ResultInternal>* got) {
  memset(pass, 0, sizeof(*pass));
  pg_result* from = plan.pass_alone ? out : pass;
  pg_status st = execute_one(seg, plan.pass_alone ? &plan.pass : &plan.base, out, nullptr);
  if (st != PG_OK) return st;
  if (!plan.pass_alone) {
    out->stats.num_entries_scanned_post_filter = out->stats.num_docs_scanned * (int64_t)plan.num_projected;
    st = execute_one(seg, &plan.pass, pass, nullptr);
    if (st != PG_OK) { pg_result_free(out); return st; }
    out->device_ms += pass->device_ms;
    if (pass->dominant_kernel_ms >= out->dominant_kernel_ms) { out->dominant_kernel_ms = pass->dominant_kernel_ms; out->dominant_kernel = pass->dominant_kernel; }
  }
  got->reset(static_cast<ResultInternal*>(from->internal));
  from->internal = nullptr;
  return PG_OK;
}
// GROUP BY: the rows of the groups the ordinary query reports (group_ids: ascending raw ids, key kind 0) out of a matrix of `rows` rows of row_len
// elements, compacted in place -- group ids ascend, so row k of the result never lies behind the matrix row it is taken from: no second buffer.
// per_row(k, row's elements) sees every kept row before it moves.  false: *bad_row is a group id outside the matrix, or out of order.
extern "C++" {      // (a template inside the C ABI's linkage block)
template <typename T, typename PerRow>
static bool keep_group_rows(const pg_result* out, std::vector<T>* matrix, int rows, size_t row_len, int64_t* bad_row, PerRow&& per_row) {
  int64_t previous = -1;
  for (int k = 0; k < out->num_groups; ++k) {
    const int64_t row = out->group_ids[k];
    if (row <= previous || row >= rows) { *bad_row = row; return false; }
    previous = row;
    const T* src = matrix->data() + (size_t)row * row_len;
    per_row(k, src);
    if (row != k) memmove(matrix->data() + (size_t)k * row_len, src, row_len * sizeof(T));
  }
  matrix->resize((size_t)out->num_groups * row_len);
  matrix->shrink_to_fit();
  return true;
}
}
struct DistinctPlan : PassPlan {
  bool from_dictionary = false;      // NonScanBasedAggregationOperator: the whole dictionary
};
static bool is_distinct_pass_function(int32_t function) { return function == PG_AGG_DISTINCTCOUNT || is_hll_function(function); }
// Every reason a DISTINCTCOUNT query is declined for, from the query and the segment's metadata alone (pg_query_check and pg_execute both
// come through here), and the two queries that answer it.
static pg_status plan_distinct(const pg_segment* seg, const pg_query* q, DistinctPlan* plan) {
  if (!g_engine.initialized) return fail(PG_ERR_NOT_INITIALIZED, "pg_init has not been called");
  const int num_cols_total = (int)seg->cols.size();
  const int na = q->num_aggregations, ng = q->num_group_by;
  const bool null_handling = (q->flags & PG_QUERY_NULL_HANDLING) != 0;
  if (na < 0 || ng < 0 || (ng > 0 && !q->group_by_columns)) return fail(PG_ERR_INVALID_ARGUMENT, "bad aggregation / group-by lists");
  if (q->num_filter_nodes > 0 && (!q->filter || !q->predicates)) return fail(PG_ERR_INVALID_ARGUMENT, "filter nodes without predicates");
  bool has_hll = false;
  for (int a = 0; a < na; ++a) has_hll |= is_hll_function(q->aggregations[a].function);
  const char* const who = has_hll ? "DISTINCTCOUNTHLL" : "DISTINCTCOUNT";      // (the messages of a query without an HLL read as they always have)
  std::vector<int> distinct_cols, raw_cols, projected;
  std::vector<std::pair<int, int>> hll_raw_slots;      // DISTINCTCOUNTHLL on raw columns: distinct (column, log2m) pairs, one register set each
  std::vector<std::pair<int, int>> hll_dict_slots;     // ... on dictionary columns: the same pairs, one fold and one register matrix each
  std::vector<int> hll_dict_cols, hll_aggs_log2m;      // ... on dictionary columns: the columns (they share distinct_cols' bitsets); every HLL aggregation's log2m
  bool plain_distinct = false;
  auto project = [&](int c) { if (std::find(projected.begin(), projected.end(), c) == projected.end()) projected.push_back(c); };
  bool only_distinct_and_count = true, nullable_input = false;
  for (int a = 0; a < na; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    if (ag.function == PG_AGG_COUNT) {
      if (null_handling && ag.column >= 0) {
        project(ag.column); only_distinct_and_count = false;
        // (AggregationPlanNode.hasNullValues :130-153 looks at COUNT's argument too: a nullable one keeps the scan)
        if (ag.column < num_cols_total) nullable_input |= seg->cols[(size_t)ag.column].d_null_bitmap != nullptr;
      }
      continue;
    }
    if (ag.column < 0 || ag.column >= num_cols_total) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation column %d out of range", ag.column);
    project(ag.column);
    nullable_input |= seg->cols[(size_t)ag.column].d_null_bitmap != nullptr;
    if (ag.function == PG_AGG_PERCENTILE) return fail(PG_ERR_UNSUPPORTED, "PERCENTILE beside %s in one query -- CPU plan", has_hll ? "DISTINCTCOUNTHLL" : "DISTINCTCOUNT");
    const bool hll = is_hll_function(ag.function);
    if (ag.function != PG_AGG_DISTINCTCOUNT && !hll) { only_distinct_and_count = false; continue; }
    const ColumnDev& col = seg->cols[(size_t)ag.column];
    // a raw column: its values are collected, sorted and run-length encoded (the collect pass); a dictionary column: its dictId bitset
    const bool raw = col.encoding != PG_FWD_FIXED_BIT_DICT;
    if (!hll && raw) { const pg_status cst = plan_collect_column(col, "DISTINCTCOUNT"); if (cst != PG_OK) return cst; }
    if (null_handling && col.d_null_bitmap != nullptr)
      return fail(PG_ERR_UNSUPPORTED, "%s on column %s, which carries a null value vector, under null handling -- CPU plan", hll ? "DISTINCTCOUNTHLL" : "DISTINCTCOUNT", col.name.c_str());
    if (hll) {
      // a raw column: one pass of scan_hll_kernel / group_hll_kernel (no switch, no sort); a dictionary column: one more user of the column's bitset
      hll_aggs_log2m.push_back(pg::hll_log2m_of(ag.function));
      if (raw) {
        if (col.encoding != PG_FWD_RAW_FIXED_BYTE || col.stored_type < PG_TYPE_INT || col.stored_type > PG_TYPE_DOUBLE || col.d_fwd == nullptr)
          return fail(PG_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL on column %s: neither dictionary-encoded nor raw fixed-width INT / LONG / FLOAT / DOUBLE -- CPU plan", col.name.c_str());
        const std::pair<int, int> slot(ag.column, hll_aggs_log2m.back());
        if (std::find(hll_raw_slots.begin(), hll_raw_slots.end(), slot) == hll_raw_slots.end()) hll_raw_slots.push_back(slot);
        continue;
      }
      if (std::find(hll_dict_cols.begin(), hll_dict_cols.end(), ag.column) == hll_dict_cols.end()) hll_dict_cols.push_back(ag.column);
      const std::pair<int, int> slot(ag.column, hll_aggs_log2m.back());
      if (std::find(hll_dict_slots.begin(), hll_dict_slots.end(), slot) == hll_dict_slots.end()) hll_dict_slots.push_back(slot);
    } else {
      plain_distinct = true;
    }
    std::vector<int>& into = raw ? raw_cols : distinct_cols;
    if (std::find(into.begin(), into.end(), ag.column) == into.end()) into.push_back(ag.column);
  }
  if (!raw_cols.empty() && !distinct_cols.empty())
    return fail(PG_ERR_UNSUPPORTED, "DISTINCTCOUNT on raw column %s and dictionary column %s in one query -- CPU plan", seg->cols[(size_t)raw_cols[0]].name.c_str(), seg->cols[(size_t)distinct_cols[0]].name.c_str());
  if (!hll_raw_slots.empty() && !hll_dict_cols.empty())
    return fail(PG_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL on raw column %s and dictionary column %s in one query -- CPU plan", seg->cols[(size_t)hll_raw_slots[0].first].name.c_str(), seg->cols[(size_t)hll_dict_cols[0]].name.c_str());
  if (!hll_raw_slots.empty() && plain_distinct)
    return fail(PG_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL on raw column %s beside a DISTINCTCOUNT in one query -- CPU plan", seg->cols[(size_t)hll_raw_slots[0].first].name.c_str());
  if ((int)(distinct_cols.size() + raw_cols.size()) > kMaxAggCols || (int)hll_raw_slots.size() > kMaxAggCols || (int)hll_dict_slots.size() > kMaxAggCols)
    return fail(PG_ERR_UNSUPPORTED, has_hll ? "more than %d DISTINCTCOUNTHLL columns" : "more than %d DISTINCTCOUNT columns", kMaxAggCols);
  bool match_all = false, filter_stages_set = false;
  pg_status st = plan_pass_filter(seg, q, who, &match_all, &filter_stages_set); if (st != PG_OK) return st;
  if (ng > 0) {
    // GROUP BY, first cut: the key space, then the bit matrices within the cap -- priced with the functions the pass allocates by (pg_set_pass_layout.h)
    unsigned long long product = 1;
    st = plan_pass_keys(seg, q, who, &projected, &product); if (st != PG_OK) return st;
    SetMatrixLayout bitsets;
    for (int c : distinct_cols) bitsets.add(false, product, seg->cols[(size_t)c].bits, seg->cols[(size_t)c].cardinality);
    const unsigned long long matrix = bitsets.total_words() * 4ull;      // (the room behind the last row is part of the device allocation)
    if (matrix > PG_DISTINCT_GROUP_MAX_BYTES)
      return fail(PG_ERR_UNSUPPORTED, "DISTINCTCOUNT bit matrices of %llu bytes exceed PG_DISTINCT_GROUP_MAX_BYTES (%llu) -- CPU plan", matrix, (unsigned long long)PG_DISTINCT_GROUP_MAX_BYTES);
    if (matrix > g_engine.group_table_bytes)
      return fail(PG_ERR_UNSUPPORTED, "DISTINCTCOUNT bit matrices of %llu bytes exceed the %llu-byte budget (PINOT_GPU_GROUP_TABLE_BYTES)", matrix, (unsigned long long)g_engine.group_table_bytes);
    // the register matrices: one row of 2^log2m staged 32-bit words per raw group id -- per HLL aggregation (dictionary form) or per slot (raw form)
    unsigned long long registers = 0;
    for (const auto& slot : !hll_raw_slots.empty() ? hll_raw_slots : hll_dict_slots) registers += hll_staged_words(product, slot.second) * 4ull;
    if (registers > PG_HLL_GROUP_MAX_BYTES)
      return fail(PG_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL register matrices of %llu bytes exceed PG_HLL_GROUP_MAX_BYTES (%llu) -- CPU plan", registers, (unsigned long long)PG_HLL_GROUP_MAX_BYTES);
    if (registers > g_engine.group_table_bytes)
      return fail(PG_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL register matrices of %llu bytes exceed the %llu-byte budget (PINOT_GPU_GROUP_TABLE_BYTES)", registers, (unsigned long long)g_engine.group_table_bytes);
  } else if (!hll_raw_slots.empty()) {
    // scan_hll_kernel keeps every slot's registers in LDS beside the filter's staged set area and the reduction records: there is no HBM tier
    size_t lds = 0;
    for (const auto& slot : hll_raw_slots) lds += (size_t)4 << slot.second;
    if (filter_stages_set && g_engine.set_lds) lds += (size_t)kSetLdsWords * 4;
    if (std::max(lds, kCountsRecordBytes) > kLdsBudget)
      return fail(PG_ERR_UNSUPPORTED, "DISTINCTCOUNTHLL registers of %zu bytes (with the filter's set area) exceed the %zu bytes of LDS a workgroup has -- CPU plan", lds, kLdsBudget);
  }
  plan->num_projected = (int)projected.size();
  int32_t pass_flags = kQueryDistinctPass;
  if (!raw_cols.empty()) {
    st = plan_collect_bytes(seg, "DISTINCTCOUNT", raw_cols.size(), ng > 0); if (st != PG_OK) return st;
    pass_flags |= kQueryCollectPass;
  }
  if (!hll_raw_slots.empty()) pass_flags |= kQueryHllPass;
  // the dictionary answers under the conditions of the MIN / MAX dictionary path (answer_from_metadata): every function of the query that way
  // (a raw column has no dictionary to read: it is always scanned)
  plan->from_dictionary = ng == 0 && match_all && !(null_handling && nullable_input) && raw_cols.empty() && hll_raw_slots.empty();
  for (int a = 0; a < na && plan->from_dictionary; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    plan->from_dictionary = ag.function == PG_AGG_COUNT || is_distinct_pass_function(ag.function) ||
                            ((ag.function == PG_AGG_MIN || ag.function == PG_AGG_MAX) && seg->cols[(size_t)ag.column].encoding == PG_FWD_FIXED_BIT_DICT);
  }
  plan->pass_alone = ng == 0 && !plan->from_dictionary && only_distinct_and_count;
  return split_pass_query(seg, q, plan, is_distinct_pass_function, pass_flags, !plan->from_dictionary);
}
static void distinct_agg_value(pg_agg_value* v, int64_t cardinality) { memset(v, 0, sizeof(*v)); empty_agg_value(v, cardinality); }

static pg_status execute_distinct(pg_segment* seg, const pg_query* q, pg_result* out) {
  if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "null result");
  memset(out, 0, sizeof(*out));
  if (!seg || !q) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  DistinctPlan plan;
  pg_status st = plan_distinct(seg, q, &plan);
  if (st != PG_OK) return st;
  const int na = q->num_aggregations;
  if (plan.pass_alone) return execute_one(seg, &plan.pass, out, nullptr);
  std::unique_ptr<ResultInternal> sets(new ResultInternal());
  if (plan.from_dictionary) {
    st = execute_one(seg, &plan.base, out, nullptr); if (st != PG_OK) return st;
    out->stats.num_entries_scanned_post_filter = 0;
    for (int a = 0; a < na; ++a) {
      if (is_hll_function(q->aggregations[a].function)) {
        // the whole dictionary folded into registers (the reference converts the dictionary's values; nothing is scanned)
        const ColumnDev& col = seg->cols[(size_t)q->aggregations[a].column];
        HllSet hs;
        hs.aggregation = a; hs.log2m = pg::hll_log2m_of(q->aggregations[a].function); hs.rows = 1;
        hs.registers.assign((size_t)1 << hs.log2m, 0);
        for (int d = 0; d < col.cardinality; ++d) {
          uint64_t v;
          if (col.vkind != kValF64) v = (uint64_t)col.h_dict_i64[(size_t)d];
          else { memcpy(&v, &col.h_dict_f64[(size_t)d], 8); if (col.stored_type == PG_TYPE_FLOAT) v = pg::hll_long_of_bits32(pg::hll_float_bits_of_widened(v)); }
          const uint32_t x = pg::hll_hash_long(v);
          uint8_t& reg = hs.registers[pg::hll_index(x, hs.log2m)];
          reg = std::max(reg, (uint8_t)pg::hll_rank(x, hs.log2m));
        }
        distinct_agg_value(&out->aggregations[a], hll_nonzero(hs.registers.data(), hs.registers.size()));
        sets->hll.push_back(std::move(hs));
        continue;
      }
      if (q->aggregations[a].function != PG_AGG_DISTINCTCOUNT) continue;
      const int card = seg->cols[(size_t)q->aggregations[a].column].cardinality;
      DistinctSet ds;
      ds.aggregation = a; ds.num_words = (card + 31) / 32;
      ds.words.assign((size_t)ds.num_words, 0xFFFFFFFFu);
      if (card & 31) ds.words.back() = (1u << (card & 31)) - 1u;
      distinct_agg_value(&out->aggregations[a], card);
      sets->distinct.push_back(std::move(ds));
    }
    out->internal = sets.release();
    return PG_OK;
  }
  pg_result pass;
  std::unique_ptr<ResultInternal> got;
  st = execute_base_and_pass(seg, plan, out, &pass, &got); if (st != PG_OK) return st;
  if (!got) { pg_result_free(&pass); pg_result_free(out); return fail(PG_ERR_INTERNAL, "the DISTINCTCOUNT pass returned no sets"); }
  if (!got->values.empty()) {
    // raw columns: sorted runs instead of bitsets
    if (q->num_group_by == 0) for (const ValueList& vl : got->values) out->aggregations[vl.aggregation] = pass.aggregations[vl.aggregation];
    pg_result_free(&pass);
    st = finish_value_lists(q, out, got.get(), PG_AGG_DISTINCTCOUNT);
    if (st != PG_OK) { pg_result_free(out); return st; }
    out->internal = got.release();
    return PG_OK;
  }
  if (q->num_group_by == 0) {
    for (const DistinctSet& ds : got->distinct) out->aggregations[ds.aggregation] = pass.aggregations[ds.aggregation];
    for (const HllSet& hs : got->hll) out->aggregations[hs.aggregation] = pass.aggregations[hs.aggregation];
    out->internal = got.release();
    pg_result_free(&pass);
    return PG_OK;
  }
  pg_result_free(&pass);
  // GROUP BY: the rows of the groups the ordinary query reports out of each matrix
  int64_t bad_row = 0;
  for (DistinctSet& m : got->distinct) {
    const bool kept = keep_group_rows(out, &m.words, m.rows, (size_t)m.num_words, &bad_row, [&](int k, const uint32_t* row) {
      int64_t card = 0;
      for (int w = 0; w < m.num_words; ++w) card += __builtin_popcount(row[w]);
      distinct_agg_value(&out->group_aggregations[(size_t)k * (size_t)na + (size_t)m.aggregation], card);
    });
    if (!kept) { pg_result_free(out); return fail(PG_ERR_INTERNAL, "group id %lld outside the DISTINCTCOUNT matrix of %d rows, or out of order", (long long)bad_row, m.rows); }
    m.rows = out->num_groups;
    sets->distinct.push_back(std::move(m));
  }
  for (HllSet& m : got->hll) {
    const size_t m_regs = (size_t)1 << m.log2m;
    const bool kept = keep_group_rows(out, &m.registers, m.rows, m_regs, &bad_row, [&](int k, const uint8_t* row) {
      distinct_agg_value(&out->group_aggregations[(size_t)k * (size_t)na + (size_t)m.aggregation], hll_nonzero(row, m_regs));
    });
    if (!kept) { pg_result_free(out); return fail(PG_ERR_INTERNAL, "group id %lld outside the DISTINCTCOUNTHLL matrix of %d rows, or out of order", (long long)bad_row, m.rows); }
    m.rows = out->num_groups;
    sets->hll.push_back(std::move(m));
  }
  out->internal = sets.release();
  return PG_OK;
}

// ---- PG_AGG_VARIANCE: VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP as VarianceTuple(count, sum, m2) (pg_scan_moments.h) ----
// Two runs over the same filter, on the same stream one after the other:
//   the ordinary query  -- the caller's list with every VARIANCE turned into AVG on the same column: count and sum per row, every other function,
//                          the statistics and (GROUP BY) the list of groups come from the paths they take today, untouched;
//   the moments pass    -- everything BUT the VARIANCEs turned into COUNT(*), flagged kQueryDistinctPass | kQueryMomentsPass: one launch of
//                          scan_moments_kernel / group_moments_kernel behind the same lowered filter, accumulating S1 = sum(x - c) and
//                          S2 = sum((x - c)^2) around the pivot c = sum / count of every (row, column).
// m2 = S2 - S1^2 / n: exact in exact arithmetic for ANY c; with c the row's own mean up to SUM's rounding, S1 is small and S2 a sum of non-negative
// terms of the spread's own size -- where VarianceTuple.apply(double) (:35-42) subtracts numbers of the values' size.  There is no metadata fast
// path (the reference always scans) and the pass never runs alone.  A row or query without a doc: m2 = 0, nothing launched for it.
static bool has_moments(const pg_query* q) {
  if (!q || !q->aggregations) return false;
  for (int a = 0; a < q->num_aggregations; ++a) if (is_moments_function(q->aggregations[a].function)) return true;
  return false;
}
struct MomentsPlan : PassPlan {
  std::vector<int> cols;             // the distinct VARIANCE columns, in first-use order (the pass binds them in the same order)
  unsigned long long rows = 1;       // GROUP BY: raw group ids
};
// Every reason a VARIANCE query is declined for, from the query and the segment's metadata alone (pg_query_check and pg_execute both come
// through here), and the two queries that answer it.
static pg_status plan_moments(const pg_segment* seg, const pg_query* q, MomentsPlan* plan) {
  if (!g_engine.initialized) return fail(PG_ERR_NOT_INITIALIZED, "pg_init has not been called");
  const int num_cols_total = (int)seg->cols.size();
  const int na = q->num_aggregations, ng = q->num_group_by;
  const bool null_handling = (q->flags & PG_QUERY_NULL_HANDLING) != 0;
  if (na < 0 || ng < 0 || (ng > 0 && !q->group_by_columns)) return fail(PG_ERR_INVALID_ARGUMENT, "bad aggregation / group-by lists");
  if (q->num_filter_nodes > 0 && (!q->filter || !q->predicates)) return fail(PG_ERR_INVALID_ARGUMENT, "filter nodes without predicates");
  std::vector<int> projected;
  auto project = [&](int c) { if (std::find(projected.begin(), projected.end(), c) == projected.end()) projected.push_back(c); };
  for (int a = 0; a < na; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    if (ag.function == PG_AGG_COUNT) { if (null_handling && ag.column >= 0) project(ag.column); continue; }
    if (ag.function == PG_AGG_DISTINCTCOUNT || ag.function == PG_AGG_PERCENTILE || is_hll_function(ag.function))
      return fail(PG_ERR_UNSUPPORTED, "%s beside VARIANCE in one query -- CPU plan", ag.function == PG_AGG_PERCENTILE ? "PERCENTILE" : (ag.function == PG_AGG_DISTINCTCOUNT ? "DISTINCTCOUNT" : "DISTINCTCOUNTHLL"));
    if (ag.column < 0 || ag.column >= num_cols_total) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation column %d out of range", ag.column);
    project(ag.column);
    if (!is_moments_function(ag.function)) continue;
    const ColumnDev& col = seg->cols[(size_t)ag.column];
    if (null_handling && col.d_null_bitmap != nullptr)
      return fail(PG_ERR_UNSUPPORTED, "VARIANCE on column %s, which carries a null value vector, under null handling -- CPU plan", col.name.c_str());
    const bool dict = col.encoding == PG_FWD_FIXED_BIT_DICT;
    if ((!dict && col.encoding != PG_FWD_RAW_FIXED_BYTE) || col.stored_type < PG_TYPE_INT || col.stored_type > PG_TYPE_DOUBLE || col.d_fwd == nullptr ||
        (dict && (col.vkind == kValI32 ? (const void*)col.d_dict : (const void*)col.d_dict64) == nullptr))
      return fail(PG_ERR_UNSUPPORTED, "VARIANCE on column %s: neither a dictionary-encoded nor a raw fixed-width INT / LONG / FLOAT / DOUBLE column -- CPU plan", col.name.c_str());
    // GROUP BY on a raw LONG column: the ordinary query's table slot is one wrapping int64 (a dictionary column of such values is declined by the
    // ordinary query itself).  moments_pivot undoes a wrap while numDocs x (max - min) stays below 2^64; beyond that no pivot can be trusted.
    if (ng > 0 && !dict && col.stored_type == PG_TYPE_LONG && col.raw_max >= col.raw_min &&
        (double)seg->num_docs * std::max(std::fabs((double)col.raw_min), std::fabs((double)col.raw_max)) >= 9.2e18 &&
        (double)seg->num_docs * ((double)col.raw_max - (double)col.raw_min) >= 1.8e19)
      return fail(PG_ERR_UNSUPPORTED, "VARIANCE grouped on raw LONG column %s, whose group sums could wrap int64 beyond repair -- CPU plan", col.name.c_str());
    if (std::find(plan->cols.begin(), plan->cols.end(), ag.column) == plan->cols.end()) plan->cols.push_back(ag.column);
  }
  if ((int)plan->cols.size() > kMaxAggCols) return fail(PG_ERR_UNSUPPORTED, "more than %d VARIANCE columns -- CPU plan", kMaxAggCols);
  bool match_all = false, filter_stages_set = false;
  pg_status st = plan_pass_filter(seg, q, "VARIANCE", &match_all, &filter_stages_set); if (st != PG_OK) return st;
  if (ng > 0) {
    st = plan_pass_keys(seg, q, "VARIANCE", &projected, &plan->rows); if (st != PG_OK) return st;
    // S1, S2 and the pivot of every (raw group id, column)
    const unsigned long long matrix = plan->rows * 24ull * (unsigned long long)plan->cols.size();
    if (matrix > PG_MOMENTS_GROUP_MAX_BYTES)
      return fail(PG_ERR_UNSUPPORTED, "VARIANCE moment matrices of %llu bytes exceed PG_MOMENTS_GROUP_MAX_BYTES (%llu) -- CPU plan", matrix, (unsigned long long)PG_MOMENTS_GROUP_MAX_BYTES);
    if (matrix > g_engine.group_table_bytes)
      return fail(PG_ERR_UNSUPPORTED, "VARIANCE moment matrices of %llu bytes exceed the %llu-byte budget (PINOT_GPU_GROUP_TABLE_BYTES) -- CPU plan", matrix, (unsigned long long)g_engine.group_table_bytes);
  }
  plan->num_projected = (int)projected.size();
  plan->pass_alone = false;
  return split_pass_query(seg, q, plan, is_moments_function, kQueryDistinctPass | kQueryMomentsPass, true, PG_AGG_AVG);
}
// m2 of n values from the pivoted moments.  Rounding can leave it a hair below zero (a constant column): raised to 0.  NaN stays NaN -- a NaN or an
// infinity among the values makes sum, the pivot and both moments non-finite, as it makes the reference's m2 (inf - inf).
static double moments_m2(double s1, double s2, int64_t n) {
  if (n <= 0) return 0.0;
  const double m2 = s2 - s1 * s1 / (double)n;
  return m2 < 0.0 ? 0.0 : m2;
}
// The pivot of one row: sum / count as a double.  A group-by's SUM of a raw LONG column is an int64 that wraps without telling (the aggregation-only
// path reports the double image of a wrapped sum instead); the true sum lies in [count x min, count x max] of the column, and plan_moments kept
// that interval narrower than 2^64: the one multiple of 2^64 that brings the sum back into it is added here.  (pg_agg_value.sum itself stays what
// PG_AGG_SUM reports.)
static double moments_pivot(const ColumnDev& col, const pg_agg_value& v, bool grouped) {
  if (grouped && col.encoding == PG_FWD_RAW_FIXED_BYTE && col.stored_type == PG_TYPE_LONG && col.raw_max >= col.raw_min) {
    const __int128 lo = (__int128)v.count * (__int128)col.raw_min, hi = (__int128)v.count * (__int128)col.raw_max, wrap = (__int128)1 << 64;
    __int128 s = (__int128)v.sum_i64;
    if (s < lo) s += (lo - s + wrap - 1) / wrap * wrap;
    else if (s > hi) s -= (s - hi + wrap - 1) / wrap * wrap;
    return (double)s / (double)v.count;
  }
  return v.sum / (double)v.count;
}
static void moments_agg_value(pg_agg_value* v) { v->min = std::numeric_limits<double>::infinity(); v->max = -std::numeric_limits<double>::infinity(); }

static pg_status execute_moments(pg_segment* seg, const pg_query* q, pg_result* out) {
  if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "null result");
  memset(out, 0, sizeof(*out));
  if (!seg || !q) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  MomentsPlan plan;
  pg_status st = plan_moments(seg, q, &plan);
  if (st != PG_OK) return st;
  const int na = q->num_aggregations;
  const bool grouped = q->num_group_by > 0;
  const size_t cols = plan.cols.size();
  // 1. the ordinary query: count and sum per row
  st = execute_one(seg, &plan.base, out, nullptr); if (st != PG_OK) return st;
  if (grouped && out->group_key_kind != 0) { pg_result_free(out); return fail(PG_ERR_INTERNAL, "VARIANCE: the ordinary query grouped over a key space of kind %d", (int)out->group_key_kind); }
  // 2. the pivots, by raw group id (rows without a doc keep 0)
  std::vector<int> col_of((size_t)std::max(na, 1), -1);
  for (int a = 0; a < na; ++a)
    if (is_moments_function(q->aggregations[a].function)) col_of[(size_t)a] = (int)(std::find(plan.cols.begin(), plan.cols.end(), q->aggregations[a].column) - plan.cols.begin());
  std::vector<double> pivots((size_t)plan.rows * cols, 0.0);
  bool any = false;
  const int num_rows_out = grouped ? out->num_groups : 1;
  for (int k = 0; k < num_rows_out; ++k) {
    const int64_t row = grouped ? out->group_ids[k] : 0;
    if (row < 0 || (unsigned long long)row >= plan.rows) { pg_result_free(out); return fail(PG_ERR_INTERNAL, "group id %lld outside the VARIANCE matrix of %llu rows", (long long)row, plan.rows); }
    for (int a = 0; a < na; ++a) {
      if (col_of[(size_t)a] < 0) continue;
      pg_agg_value* v = grouped ? &out->group_aggregations[(size_t)k * (size_t)na + (size_t)a] : &out->aggregations[a];
      moments_agg_value(v);
      if (v->count > 0) { pivots[(size_t)row * cols + (size_t)col_of[(size_t)a]] = moments_pivot(seg->cols[(size_t)q->aggregations[a].column], *v, grouped); any = true; }
    }
  }
  std::unique_ptr<ResultInternal> sets(new ResultInternal());
  if (!any) {
    // no doc behind the filter: every tuple is (0, 0, 0), nothing is launched
    for (int a = 0; a < na; ++a) {
      if (col_of[(size_t)a] < 0) continue;
      MomentsSet ms;
      ms.aggregation = a; ms.rows = num_rows_out; ms.m2.assign((size_t)num_rows_out, 0.0);
      sets->moments.push_back(std::move(ms));
    }
    out->internal = sets.release();
    return PG_OK;
  }
  // 3. the moments pass behind the same filter
  pg_result pass;
  memset(&pass, 0, sizeof(pass));
  t_moments_pivots = &pivots;
  st = execute_one(seg, &plan.pass, &pass, nullptr);
  t_moments_pivots = nullptr;
  if (st != PG_OK) { pg_result_free(out); return st; }
  out->device_ms += pass.device_ms;
  if (pass.dominant_kernel_ms >= out->dominant_kernel_ms) { out->dominant_kernel_ms = pass.dominant_kernel_ms; out->dominant_kernel = pass.dominant_kernel; }
  std::unique_ptr<ResultInternal> got(static_cast<ResultInternal*>(pass.internal));
  pass.internal = nullptr;
  const int64_t pass_docs = pass.stats.num_docs_scanned;
  pg_result_free(&pass);
  if (!got || got->moments.empty()) { pg_result_free(out); return fail(PG_ERR_INTERNAL, "the VARIANCE pass returned no moments"); }
  if (pass_docs != out->stats.num_docs_scanned) { pg_result_free(out); return fail(PG_ERR_INTERNAL, "the VARIANCE pass saw %lld docs, the ordinary query %lld", (long long)pass_docs, (long long)out->stats.num_docs_scanned); }
  // 4. the harvest: m2 per row (GROUP BY: the rows of the groups the ordinary query reports)
  for (MomentsSet& m : got->moments) {
    if (!grouped) {
      if (m.m2.size() != 2) { pg_result_free(out); return fail(PG_ERR_INTERNAL, "VARIANCE: %zu moments for one row", m.m2.size()); }
      m.m2 = {moments_m2(m.m2[0], m.m2[1], out->aggregations[m.aggregation].count)};
      m.rows = 1;
    } else {
      std::vector<double> m2((size_t)out->num_groups, 0.0);
      int64_t bad_row = 0;
      const bool kept = keep_group_rows(out, &m.m2, m.rows, 2, &bad_row, [&](int k, const double* row) {
        m2[(size_t)k] = moments_m2(row[0], row[1], out->group_aggregations[(size_t)k * (size_t)na + (size_t)m.aggregation].count);
      });
      if (!kept) { pg_result_free(out); return fail(PG_ERR_INTERNAL, "group id %lld outside the VARIANCE matrix of %d rows, or out of order", (long long)bad_row, m.rows); }
      m.m2 = std::move(m2);
      m.rows = out->num_groups;
    }
    sets->moments.push_back(std::move(m));
  }
  out->internal = sets.release();
  return PG_OK;
}

// ---- PG_AGG_PERCENTILE: the dictId count histograms of dictionary columns (pg_scan_counts.h) ----
// The DISTINCTCOUNT scheme with counters: the ordinary query (every PERCENTILE turned into COUNT(*)) brings every other function, the statistics
// and the list of groups; the counts pass (everything BUT the PERCENTILEs turned into COUNT(*), flagged kQueryCountsPass) is one launch of
// scan_counts_kernel / group_counts_kernel behind the same lowered filter.  `PERCENTILE(c1..c4) [, COUNT(*)]` without GROUP BY is the pass alone.
// There is no metadata fast path: the reference scans even without a filter (its plain golden's statistics are (docs, 0, docs x columns, docs)).
// The percentile itself is not part of the query: the list is the intermediate result whatever p is.
static bool has_percentile(const pg_query* q) {
  if (!q || !q->aggregations) return false;
  for (int a = 0; a < q->num_aggregations; ++a) if (q->aggregations[a].function == PG_AGG_PERCENTILE) return true;
  return false;
}
struct PercentilePlan : PassPlan {};
static bool is_percentile_function(int32_t function) { return function == PG_AGG_PERCENTILE; }
// Every reason a PERCENTILE query is declined for, from the query and the segment's metadata alone (pg_query_check and pg_execute both come
// through here), and the two queries that answer it.
static pg_status plan_percentile(const pg_segment* seg, const pg_query* q, PercentilePlan* plan) {
  if (!g_engine.initialized) return fail(PG_ERR_NOT_INITIALIZED, "pg_init has not been called");
  const int num_cols_total = (int)seg->cols.size();
  const int na = q->num_aggregations, ng = q->num_group_by;
  const bool null_handling = (q->flags & PG_QUERY_NULL_HANDLING) != 0;
  if (na < 0 || ng < 0 || (ng > 0 && !q->group_by_columns)) return fail(PG_ERR_INVALID_ARGUMENT, "bad aggregation / group-by lists");
  if (q->num_filter_nodes > 0 && (!q->filter || !q->predicates)) return fail(PG_ERR_INVALID_ARGUMENT, "filter nodes without predicates");
  std::vector<int> pct_cols, raw_cols, projected;
  auto project = [&](int c) { if (std::find(projected.begin(), projected.end(), c) == projected.end()) projected.push_back(c); };
  bool only_percentile_and_count = true;
  for (int a = 0; a < na; ++a) {
    const pg_aggregation& ag = q->aggregations[a];
    if (ag.function == PG_AGG_DISTINCTCOUNT) return fail(PG_ERR_UNSUPPORTED, "PERCENTILE beside DISTINCTCOUNT in one query -- CPU plan");
    if (is_hll_function(ag.function)) return fail(PG_ERR_UNSUPPORTED, "PERCENTILE beside DISTINCTCOUNTHLL in one query -- CPU plan");
    if (ag.function == PG_AGG_COUNT) {
      if (null_handling && ag.column >= 0) { project(ag.column); only_percentile_and_count = false; }
      continue;
    }
    if (ag.column < 0 || ag.column >= num_cols_total) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation column %d out of range", ag.column);
    project(ag.column);
    if (ag.function != PG_AGG_PERCENTILE) { only_percentile_and_count = false; continue; }
    const ColumnDev& col = seg->cols[(size_t)ag.column];
    // a raw column: its values are collected, sorted and run-length encoded (the collect pass); a dictionary column: its dictId counters
    const bool raw = col.encoding != PG_FWD_FIXED_BIT_DICT;
    if (raw) { const pg_status cst = plan_collect_column(col, "PERCENTILE"); if (cst != PG_OK) return cst; }
    if (null_handling && col.d_null_bitmap != nullptr)
      return fail(PG_ERR_UNSUPPORTED, "PERCENTILE on column %s, which carries a null value vector, under null handling -- CPU plan", col.name.c_str());
    std::vector<int>& into = raw ? raw_cols : pct_cols;
    if (std::find(into.begin(), into.end(), ag.column) == into.end()) into.push_back(ag.column);
  }
  if (!raw_cols.empty() && !pct_cols.empty())
    return fail(PG_ERR_UNSUPPORTED, "PERCENTILE on raw column %s and dictionary column %s in one query -- CPU plan", seg->cols[(size_t)raw_cols[0]].name.c_str(), seg->cols[(size_t)pct_cols[0]].name.c_str());
  if ((int)(pct_cols.size() + raw_cols.size()) > kMaxAggCols) return fail(PG_ERR_UNSUPPORTED, "more than %d PERCENTILE columns", kMaxAggCols);
  bool match_all = false, filter_stages_set = false;      // (no metadata fast path and no LDS-only tier here: neither is read)
  pg_status st = plan_pass_filter(seg, q, "PERCENTILE", &match_all, &filter_stages_set); if (st != PG_OK) return st;
  if (ng > 0) {
    // GROUP BY under plan_distinct's conditions.  The counter matrices: group_id_upper_bound x cardinality x 4 bytes per column, and behind the last
    // counter the 2^bits - cardinality counters a dictId beyond the dictionary's bound could reach -- priced with the functions the pass allocates
    // by (pg_set_pass_layout.h)
    unsigned long long product = 1;
    st = plan_pass_keys(seg, q, "PERCENTILE", &projected, &product); if (st != PG_OK) return st;
    SetMatrixLayout counters;
    for (int c : pct_cols) counters.add(true, product, seg->cols[(size_t)c].bits, seg->cols[(size_t)c].cardinality);
    const unsigned long long matrix = counters.total_words() * 4ull;
    if (matrix > PG_PERCENTILE_GROUP_MAX_BYTES)
      return fail(PG_ERR_UNSUPPORTED, "PERCENTILE counter matrices of %llu bytes exceed PG_PERCENTILE_GROUP_MAX_BYTES (%llu) -- CPU plan", matrix, (unsigned long long)PG_PERCENTILE_GROUP_MAX_BYTES);
    if (matrix > g_engine.group_table_bytes)
      return fail(PG_ERR_UNSUPPORTED, "PERCENTILE counter matrices of %llu bytes exceed the %llu-byte budget (PINOT_GPU_GROUP_TABLE_BYTES)", matrix, (unsigned long long)g_engine.group_table_bytes);
  }
  plan->num_projected = (int)projected.size();
  int32_t pass_flags = kQueryCountsPass;
  if (!raw_cols.empty()) {
    st = plan_collect_bytes(seg, "PERCENTILE", raw_cols.size(), ng > 0); if (st != PG_OK) return st;
    pass_flags |= kQueryCollectPass;
  }
  plan->pass_alone = ng == 0 && only_percentile_and_count;
  return split_pass_query(seg, q, plan, is_percentile_function, pass_flags);
}

// Row `row` of a dense counter matrix -> the pairs of a CountList; returns the docs counted.
static int64_t append_count_row(CountList* list, const uint32_t* dense, int cardinality) {
  int64_t docs = 0;
  for (int d = 0; d < cardinality; ++d) {
    if (dense[d] == 0u) continue;
    list->dict_ids.push_back(d);
    list->counts.push_back(dense[d]);
    docs += dense[d];
  }
  list->offsets.push_back(list->dict_ids.size());
  return docs;
}

static pg_status execute_percentile(pg_segment* seg, const pg_query* q, pg_result* out) {
  if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "null result");
  memset(out, 0, sizeof(*out));
  if (!seg || !q) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  PercentilePlan plan;
  pg_status st = plan_percentile(seg, q, &plan);
  if (st != PG_OK) return st;
  const int na = q->num_aggregations;
  pg_result pass;
  std::unique_ptr<ResultInternal> got;
  st = execute_base_and_pass(seg, plan, out, &pass, &got); if (st != PG_OK) return st;
  pg_result_free(&pass);
  auto give_up = [&](const char* what) { pg_result_free(out); memset(out, 0, sizeof(*out)); return fail(PG_ERR_INTERNAL, "%s", what); };
  if (!got) return give_up("the PERCENTILE pass returned no counters");
  if (!got->values.empty()) {
    // raw columns: the pass's sorted runs are the list (aggregation only: convert left the docs aggregated in every PERCENTILE's count)
    st = finish_value_lists(q, out, got.get(), PG_AGG_PERCENTILE);
    if (st != PG_OK) { pg_result_free(out); memset(out, 0, sizeof(*out)); return st; }
    out->internal = got.release();
    return PG_OK;
  }
  // the dense rows -> (dictId, count) pairs; GROUP BY: only the rows of the groups the ordinary query reports (group_ids: ascending raw ids, key kind 0)
  std::unique_ptr<ResultInternal> lists(new ResultInternal());
  const bool grouped = q->num_group_by > 0;
  for (const DistinctSet& m : got->distinct) {
    CountList list;
    list.aggregation = m.aggregation;
    list.offsets.push_back(0);
    if (!grouped) {
      const int64_t docs = append_count_row(&list, m.words.data(), m.num_words);
      memset(&out->aggregations[m.aggregation], 0, sizeof(pg_agg_value));
      empty_agg_value(&out->aggregations[m.aggregation], docs);
    } else {
      list.rows = out->num_groups;
      for (int k = 0; k < out->num_groups; ++k) {
        const int64_t row = out->group_ids[k];
        if (row < 0 || row >= m.rows) return give_up("a group id outside the PERCENTILE counter matrix");
        const int64_t docs = append_count_row(&list, m.words.data() + (size_t)row * (size_t)m.num_words, m.num_words);
        pg_agg_value* v = &out->group_aggregations[(size_t)k * (size_t)na + (size_t)m.aggregation];
        memset(v, 0, sizeof(*v));
        empty_agg_value(v, docs);
      }
    }
    list.dict_ids.shrink_to_fit(); list.counts.shrink_to_fit();
    lists->counts.push_back(std::move(list));
  }
  got.reset();      // (the dense matrices end here)
  out->internal = lists.release();
  return PG_OK;
}

// (pg_execute: below, behind the batch machinery -- a small group-by runs as a one-item launch of the batch's group-by kernel)

// ---- pg_execute_batch ----
namespace {

// Worker threads of the library: lowering (and, for queries that cannot share the batch launch, running) the items of a batch side by
// side.  Started on first use, parked on a condition variable in between.
struct WorkerPool {
  std::mutex mu;
  std::condition_variable wake;
  std::vector<std::thread> threads;
  std::function<void(int)> job;        // job(item)
  std::atomic<int> next{0}, remaining{0}, inside{0};
  int count = 0, grain = 1, helpers = 0;
  unsigned long long generation = 0;
  std::atomic<unsigned long long> generation_hint{0};      // == generation, readable without the mutex (the helpers' spin)
  bool stop = false;

  // Items are claimed `grain` at a time with ONE atomic add (a mutex hand-off per item cost more than lowering a query: 64 items of
  // ~2 us each took 80 us on 16 threads); whoever finishes the last item ends the run.
  void drain() {
    for (;;) {
      const int first = next.fetch_add(grain, std::memory_order_relaxed);
      if (first >= count) return;
      const int last = std::min(count, first + grain);
      for (int item = first; item < last; ++item) job(item);
      remaining.fetch_sub(last - first, std::memory_order_release);
    }
  }
  // A helper that has just worked stays on its core for a moment (being woken through the condition variable costs a run ~30 us of
  // latency, and a batch's items that miss the plan cache come in bursts); kSpinNs without a new run and the helper parks.  Round 4: 1 ms
  // -> 100 us -- with the plan cache a busy server's batches rarely need the helpers at all, and a millisecond of spinning per helper
  // after every miss was a core's worth of idle work per sixteen of them.
  static constexpr long long kSpinNs = 100'000;
  void worker(int index) {
    unsigned long long seen = 0;
    bool worked = false;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      if (worked && !stop && generation == seen) {
        lk.unlock();
        const auto until = std::chrono::steady_clock::now() + std::chrono::nanoseconds(kSpinNs);
        for (int i = 0; generation_hint.load(std::memory_order_relaxed) == seen; ++i) {
          cpu_relax();
          if ((i & 255) == 255 && std::chrono::steady_clock::now() >= until) break;
        }
        lk.lock();
      }
      worked = false;
      wake.wait(lk, [&] { return stop || generation != seen; });
      if (stop) return;
      seen = generation;
      if (index >= helpers) continue;
      worked = true;
      inside.fetch_add(1, std::memory_order_acquire);
      lk.unlock();
      drain();
      inside.fetch_sub(1, std::memory_order_release);
      lk.lock();
    }
  }
  // Runs job(0 .. n) on the pool and the calling thread; returns when all are done.  `items_per_claim`: how many items a thread takes
  // at a time (1 for items that wait for the device, more for items of a few microseconds).
  void run(int n, int max_threads, int items_per_claim, std::function<void(int)> fn) {
    if (n <= 0) return;
    {
      std::unique_lock<std::mutex> lk(mu);
      const int want = std::max(0, std::min(max_threads, (n + items_per_claim - 1) / items_per_claim) - 1);
      while ((int)threads.size() < want) { const int index = (int)threads.size(); threads.emplace_back([this, index] { worker(index); }); }
      // a helper woken late for the previous run may be inside drain() (it enters under this mutex and finds nothing left): let it leave
      while (inside.load(std::memory_order_acquire) != 0) cpu_relax();
      job = std::move(fn);
      count = n; grain = std::max(1, items_per_claim); helpers = want;
      next.store(0, std::memory_order_relaxed);
      remaining.store(n, std::memory_order_relaxed);
      ++generation;
      generation_hint.store(generation, std::memory_order_relaxed);
      if (want > 0) wake.notify_all();
    }
    drain();
    // the last items are in other threads' hands for microseconds (lowering) or for a kernel's duration (worker_threads mode): spin
    // briefly, then yield; no helper may still be inside drain() when the next run rewrites job / count
    long long spins = 0;
    while (remaining.load(std::memory_order_acquire) != 0 || inside.load(std::memory_order_acquire) != 0) {
      if (++spins > 2000) std::this_thread::yield();
    }
  }
  ~WorkerPool() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    wake.notify_all();
    for (auto& t : threads) t.join();
  }
};
WorkerPool g_pool;
// The pool runs one job at a time.  A second pg_execute_batch does NOT wait for it (two queries of a server used to run one after the
// other, end to end): it lowers its items on its own thread -- microseconds each -- or, when its items run whole kernels inside their
// claim (group-bys, 1 B-row scans), on short-lived threads of its own.  The lock covers the lowering phase only; the shared launches
// and their waits run on per-call BatchCtx's outside it.
std::mutex g_pool_mu;
void run_items(int count, int threads, int items_per_claim, bool heavy, const std::function<void(int)>& fn) {
  {
    std::unique_lock<std::mutex> lk(g_pool_mu, std::try_to_lock);
    if (lk.owns_lock()) { g_pool.run(count, threads, items_per_claim, fn); return; }
  }
  const int extra = heavy ? std::min(threads, count) - 1 : 0;
  if (extra <= 0) { for (int i = 0; i < count; ++i) fn(i); return; }
  std::atomic<int> next{0};
  auto drain = [&] { for (;;) { const int i = next.fetch_add(1, std::memory_order_relaxed); if (i >= count) return; fn(i); } };
  std::vector<std::thread> own;
  for (int t = 0; t < extra; ++t) own.emplace_back(drain);
  drain();
  for (auto& t : own) t.join();
}

// Device-side state of one batch launch, reused from call to call.
struct BatchCtx {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};      // [0], [1]: around the kernel (timed runs); [2]: the group tables' copy has landed
  // pinned staging / device copy of what the launch reads: [first workgroup of every item | the items' kernel parameters], ONE
  // allocation each so that ONE copy command precedes the launch
  uint8_t* h_blob = nullptr; uint8_t* d_blob = nullptr;
  size_t items_offset = 0;
  ScanParams* h_items = nullptr; ScanParams* d_items = nullptr;
  uint32_t* h_first = nullptr; uint32_t* d_first = nullptr;
  HostRecord* h_records = nullptr; HostRecord* h_records_dev = nullptr;  // pinned, device-mapped: one folded record per item
  size_t sets_offset = 0, set_capacity = 0;    // the blob's last part: the items' dictId sets (IN lists), uploaded with the items
  uint32_t* d_done = nullptr;                                            // kFoldShards + 1 arrival counters per item
  BlockPartial* d_partials = nullptr;
  int item_capacity = 0;
  size_t partial_capacity = 0;
  unsigned long long seq = 0;
  // group-by launches (lean_kind 6): the items' table slices -- ONE device allocation, all-zero between launches, and its pinned host image
  unsigned long long* d_gtable = nullptr; unsigned long long* h_gtable = nullptr; unsigned long long* h_gtable_dev = nullptr;      // (the image is device-mapped: items publish their slices themselves)
  size_t gtable_capacity = 0;      // words
  bool gtable_dirty = false;       // a launch did not publish every item (or the copy form's memset was not enqueued): zero the whole table and the arrival counters before the next launch
};
constexpr size_t kBatchItemSlot = sizeof(GroupParams) > sizeof(ScanParams) ? sizeof(GroupParams) : sizeof(ScanParams);      // a slot of the blob holds an item of either kind
std::mutex g_batch_mu;
std::vector<BatchCtx*> g_batch_free;

void destroy_batch_ctx(BatchCtx* b) {
  if (!b) return;
  if (b->stream) (void)hipStreamSynchronize(b->stream);      // (the group-by tables are zeroed behind the answers)
  if (b->h_blob) (void)hipHostFree(b->h_blob);
  if (b->d_blob) (void)hipFree(b->d_blob);
  if (b->h_records) (void)hipHostFree(b->h_records);
  if (b->d_done) (void)hipFree(b->d_done);
  if (b->d_partials) (void)hipFree(b->d_partials);
  if (b->d_gtable) (void)hipFree(b->d_gtable);
  if (b->h_gtable) (void)hipHostFree(b->h_gtable);
  for (auto& e : b->ev) if (e) (void)hipEventDestroy(e);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
}

pg_status ensure_batch_ctx(BatchCtx* b, int items, size_t partials, size_t set_bytes = 0 /* the items' dictId sets, behind the item slots */) {
  if (!b->stream) {
    HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    for (auto& e : b->ev) HIP_TRY(hipEventCreate(&e));
  }
  if (b->item_capacity < items || b->set_capacity < set_bytes) {
    const int cap = std::max({items, b->item_capacity, 64});
    const size_t set_cap = set_bytes > b->set_capacity ? std::max<size_t>(set_bytes * 2, 64 * 1024) : b->set_capacity;
    if (b->stream) HIP_TRY(hipStreamSynchronize(b->stream));      // (nothing of the last launch may still read the blob)
    if (b->h_blob) (void)hipHostFree(b->h_blob);
    if (b->d_blob) (void)hipFree(b->d_blob);
    if (b->h_records) (void)hipHostFree(b->h_records);
    if (b->d_done) (void)hipFree(b->d_done);
    b->h_blob = nullptr; b->d_blob = nullptr; b->h_items = nullptr; b->d_items = nullptr; b->h_first = nullptr; b->d_first = nullptr; b->h_records = nullptr; b->d_done = nullptr;
    b->item_capacity = 0;
    b->items_offset = (4 * (size_t)(cap + 1) + 255) & ~(size_t)255;
    b->sets_offset = b->items_offset + kBatchItemSlot * (size_t)cap;
    const size_t blob_bytes = b->sets_offset + set_cap;
    b->set_capacity = set_cap;
    HIP_TRY(hipHostMalloc((void**)&b->h_blob, blob_bytes, hipHostMallocDefault));
    HIP_TRY(hipMalloc((void**)&b->d_blob, blob_bytes));
    memset(b->h_blob, 0, blob_bytes);
    b->h_first = reinterpret_cast<uint32_t*>(b->h_blob); b->d_first = reinterpret_cast<uint32_t*>(b->d_blob);
    b->h_items = reinterpret_cast<ScanParams*>(b->h_blob + b->items_offset); b->d_items = reinterpret_cast<ScanParams*>(b->d_blob + b->items_offset);
    HIP_TRY(hipHostMalloc((void**)&b->h_records, sizeof(HostRecord) * (size_t)cap, hipHostMallocMapped));
    memset(b->h_records, 0, sizeof(HostRecord) * (size_t)cap);
    HIP_TRY(hipHostGetDevicePointer((void**)&b->h_records_dev, b->h_records, 0));
    HIP_TRY(hipMalloc((void**)&b->d_done, (size_t)cap * (kFoldShards + 1) * kFoldStride * 4));
    HIP_TRY(hipMemsetAsync(b->d_done, 0, (size_t)cap * (kFoldShards + 1) * kFoldStride * 4, b->stream));      // ordered before the batch's launches
    b->item_capacity = cap;
  }
  if (b->partial_capacity < partials) {
    if (b->d_partials) (void)hipFree(b->d_partials);
    b->d_partials = nullptr; b->partial_capacity = 0;
    HIP_TRY(hipMalloc((void**)&b->d_partials, sizeof(BlockPartial) * partials));
    b->partial_capacity = partials;
  }
  return PG_OK;
}

// The deferred items of one device: one launch, every item folding into its own pinned record.  Two halves, so that a batch spanning
// several devices has every device's launch in flight before it waits for any (segment s on device s mod N: BaseCombineOperator.java:85-142
// runs all segments of a query on one pool): enqueue_deferred copies the items and launches, finish_deferred waits and converts.
// The plan cache of a segment (pg_segment.plan_cache): at most kPlanCacheEntries items, most recently used first.
constexpr size_t kPlanCacheEntries = 4;

// A hit hands out the item with its value planes held again; an item lowered under other engine settings, or before a plane of the
// segment came or went, is dropped.
bool cached_item(pg_segment* seg, const std::string& key, Deferred* out) {
  std::shared_ptr<const LoweredItem> item;
  {
    std::lock_guard<std::mutex> lk(seg->plan_cache_mu);
    auto& cache = seg->plan_cache;
    for (size_t i = 0; i < cache.size(); ++i) {
      if (cache[i]->key != key) continue;
      item = cache[i];
      if (i != 0) std::rotate(cache.begin(), cache.begin() + (long)i, cache.begin() + (long)i + 1);
      break;
    }
  }
  if (!item) return false;
  bool fresh = item->engine_epoch == g_engine.epoch.load(std::memory_order_acquire);
  std::vector<int> held;
  for (size_t c = 0; c < item->plane_columns.size() && fresh; ++c) {
    bool ready = false;
    if (acquire_plane(seg, item->plane_columns[c], &ready) != PG_OK || !ready) { fresh = false; break; }
    held.push_back(item->plane_columns[c]);
  }
  // (the planes are held now: the epoch cannot move under this batch for the columns the item reads)
  fresh = fresh && item->plane_epoch == seg->plane_epoch.load(std::memory_order_acquire);
  std::unique_ptr<PlaneHold> hold(new PlaneHold(seg, std::move(held)));
  if (!fresh) {
    std::lock_guard<std::mutex> lk(seg->plan_cache_mu);
    auto& cache = seg->plan_cache;
    cache.erase(std::remove(cache.begin(), cache.end(), item), cache.end());
    return false;                                   // (`hold` releases what was acquired)
  }
  out->item = std::move(item);
  out->planes = std::move(hold);
  out->cacheable = true;
  return true;
}

void remember_item(pg_segment* seg, std::string&& key, const std::shared_ptr<const OwnedQuery>& query, Deferred* d) {
  // (the item was made by this thread a moment ago and nobody else has seen it yet)
  LoweredItem* item = std::const_pointer_cast<LoweredItem>(d->item).get();
  item->query = query;
  item->key = std::move(key);
  item->engine_epoch = g_engine.epoch.load(std::memory_order_acquire);
  item->plane_epoch = seg->plane_epoch.load(std::memory_order_acquire);
  std::lock_guard<std::mutex> lk(seg->plan_cache_mu);
  auto& cache = seg->plan_cache;
  for (size_t i = 0; i < cache.size(); ++i) if (cache[i]->key == item->key) { cache.erase(cache.begin() + (long)i); break; }
  cache.insert(cache.begin(), d->item);
  if (cache.size() > kPlanCacheEntries) cache.pop_back();
}

struct DeferredLaunch {
  BatchCtx* b = nullptr;
  int device = -1, n = 0;
  BatchKind kind = BatchKind::Private;     // ScanParams.lean_kind of every item
  std::vector<int> items, blocks;
  std::vector<size_t> table_offsets;       // GroupLds: where every item's slice starts in the context's table (words)
  long long total_blocks = 0, docs = 0;
  size_t lds = 0;
  unsigned long long seq = 0;
  bool timed = false, launched = false, publish = false;      // publish: the group-by items write their slices and sequence numbers themselves
  std::chrono::steady_clock::time_point t0, t1;
  ~DeferredLaunch() { if (b) { std::lock_guard<std::mutex> lk(g_batch_mu); g_batch_free.push_back(b); } }
};

// Workgroups per item of a shared launch in proportion to its tiles (`budget` workgroups for the launch's `total_tiles`), never more than
// the item would get on its own nor one per `per_block` tiles (L->blocks; returns their sum, L->total_blocks)
static long long share_blocks(DeferredLaunch* L, const std::vector<Deferred>& defs, pg_segment* const* segments, long long total_tiles, long long budget, long long per_block) {
  L->blocks.assign((size_t)L->n, 0);
  L->total_blocks = 0;
  for (int k = 0; k < L->n; ++k) {
    const int i = L->items[(size_t)k];
    const long long tiles = doc_tiles(segments[i]), share = total_tiles > 0 ? (tiles * budget + total_tiles - 1) / total_tiles : 1;
    L->blocks[(size_t)k] = (int)std::max<long long>(1, std::min<long long>({(long long)defs[(size_t)i].item->blocks, share, (tiles + per_block - 1) / per_block}));
    L->total_blocks += L->blocks[(size_t)k];
  }
  return L->total_blocks;
}
// The group-by items of one device (BatchKind::GroupLds): one launch of group_lds_batch_kernel over the items' GroupParams, each with a slice of the
// context's table; then ONE copy of all slices to the pinned host image and a memset that leaves the table all-zero for the next launch.
// The dictId sets (IN lists) of a deferred item ride in the batch's blob: copied behind the item slots, the item's leaves pointed at the copy
// (they were lowered against the words of a context the item is no longer tied to).  *set_off: bytes of the set area used so far.
static size_t item_set_bytes(const LoweredItem& d) {
  size_t bytes = 0;
  for (const auto& sl : d.sets) bytes += ((size_t)sl.bytes + 15) & ~(size_t)15;
  return bytes;
}
static void place_item_sets(BatchCtx* b, const LoweredItem& d, ScanParams* sp, size_t* set_off) {
  for (const auto& sl : d.sets) {
    memcpy(b->h_blob + b->sets_offset + *set_off, sl.host_words, sl.bytes);
    const uint32_t* d_words = reinterpret_cast<const uint32_t*>(b->d_blob + b->sets_offset + *set_off);
    for (int nd = 0; nd < sp->num_nodes; ++nd)
      if (sp->nodes[nd].op == PG_FILTER_LEAF && sp->nodes[nd].kind == kLeafDictSet && sp->nodes[nd].set_words == sl.ctx_words) sp->nodes[nd].set_words = d_words;
    *set_off += ((size_t)sl.bytes + 15) & ~(size_t)15;
  }
}
pg_status enqueue_group_launch(DeferredLaunch* L, BatchCtx* b, std::vector<Deferred>& defs, pg_segment* const* segments) {
  const std::vector<int>& items = L->items;
  const int n = L->n;
  long long total_tiles = 0;
  size_t launch_lds = 0, table_words = 0;
  int threads = 64;
  for (int i : items) {
    const LoweredItem& d = *defs[(size_t)i].item;
    total_tiles += doc_tiles(segments[i]);
    L->docs += (long long)segments[i]->num_docs;
    launch_lds = std::max(launch_lds, d.group_lds);
    threads = std::max(threads, d.group_threads);
    table_words += d.group_table_words;
  }
  L->lds = launch_lds;
  const int wpb = threads / 64;
  int bpc = std::max(1, std::min(waves_group_lds_batch() / wpb, (int)(kLdsBudget / std::max<size_t>(launch_lds, 1))));
  if (g_engine.blocks_per_cu > 0) bpc = g_engine.blocks_per_cu;
  const std::vector<int>& blocks = L->blocks;
  share_blocks(L, defs, segments, total_tiles, (long long)segments[items[0]]->num_cus * bpc, wpb);
  size_t set_bytes = 0, set_off = 0;
  for (int i : items) set_bytes += item_set_bytes(*defs[(size_t)i].item);
  pg_status st = ensure_batch_ctx(b, n, 0, set_bytes);
  if (st != PG_OK) return st;
  if (b->gtable_capacity < table_words) {
    if (b->d_gtable) (void)hipFree(b->d_gtable);
    if (b->h_gtable) (void)hipHostFree(b->h_gtable);
    b->d_gtable = nullptr; b->h_gtable = nullptr; b->gtable_capacity = 0;
    const size_t cap = std::max(table_words, (size_t)1 << 18);
    HIP_TRY(hipMalloc((void**)&b->d_gtable, cap * 8));
    HIP_TRY(hipHostMalloc((void**)&b->h_gtable, cap * 8, hipHostMallocMapped));
    HIP_TRY(hipHostGetDevicePointer((void**)&b->h_gtable_dev, b->h_gtable, 0));
    HIP_TRY(hipMemsetAsync(b->d_gtable, 0, cap * 8, b->stream));      // ordered before the launch below
    b->gtable_capacity = cap;
    b->gtable_dirty = false;
  }
  if (b->gtable_dirty) {
    HIP_TRY(hipMemsetAsync(b->d_gtable, 0, b->gtable_capacity * 8, b->stream));
    HIP_TRY(hipMemsetAsync(b->d_done, 0, (size_t)b->item_capacity * (kFoldShards + 1) * kFoldStride * 4, b->stream));
    b->gtable_dirty = false;
  }
  // Items publish themselves (GroupParams.host_table; PINOT_GPU_GROUP_PUBLISH=0: one copy of all slices and a memset behind the launch,
  // rounds 4-6a): the last workgroup of an item writes its slice to the pinned image and its sequence number to the item's record.
  const bool publish = g_engine.group_publish;
  L->publish = publish;
  GroupParams* h_items = reinterpret_cast<GroupParams*>(b->h_blob + b->items_offset);
  GroupParams* d_items = reinterpret_cast<GroupParams*>(b->d_blob + b->items_offset);
  size_t off = 0;
  uint32_t first = 0;
  L->seq = ++b->seq;
  L->table_offsets.assign((size_t)n, 0);
  for (int k = 0; k < n; ++k) {
    const LoweredItem& d = *defs[(size_t)items[(size_t)k]].item;
    GroupParams& gp = h_items[k];                 // (the pinned copy the device reads: filled in place)
    gp = *d.gp;
    place_item_sets(b, d, &gp.scan, &set_off);
    gp.table_count = b->d_gtable + off;
    gp.table_acc = reinterpret_cast<long long*>(b->d_gtable + off + (size_t)gp.num_groups);
    if (publish) {
      gp.host_table = b->h_gtable_dev + off;
      gp.scan.done_counter = b->d_done + (size_t)k * (kFoldShards + 1) * kFoldStride;
      gp.scan.host_out = b->h_records_dev + k;
      gp.scan.host_seq = L->seq;
    }
    L->table_offsets[(size_t)k] = off;
    off += d.group_table_words;
    b->h_first[k] = first;
    first += (uint32_t)blocks[(size_t)k];
  }
  b->h_first[n] = first;
  L->timed = (g_engine.flags & PG_CFG_TIME_KERNELS) != 0;
  L->t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipMemcpyAsync(b->d_blob, b->h_blob, b->items_offset + sizeof(GroupParams) * (size_t)n, hipMemcpyHostToDevice, b->stream));
  if (set_off) HIP_TRY(hipMemcpyAsync(b->d_blob + b->sets_offset, b->h_blob + b->sets_offset, set_off, hipMemcpyHostToDevice, b->stream));
  if (L->timed) HIP_TRY(hipEventRecord(b->ev[0], b->stream));
  b->gtable_dirty = true;
  launch_group_lds_batch((int)L->total_blocks, threads, launch_lds, b->stream, d_items, b->d_first, n);
  HIP_TRY(hipGetLastError());
  if (L->timed) HIP_TRY(hipEventRecord(b->ev[1], b->stream));
  if (publish) b->gtable_dirty = false;          // (the launch leaves table and counters as it found them; finish_group_launch says otherwise when an item stays silent)
  if (publish) (void)hipStreamQuery(b->stream);      // (nothing else of this call touches the stream before the items' numbers arrive: hand the commands to the device now)
  if (!publish) {
    HIP_TRY(hipMemcpyAsync(b->h_gtable, b->d_gtable, off * 8, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipEventRecord(b->ev[2], b->stream));
    HIP_TRY(hipMemsetAsync(b->d_gtable, 0, off * 8, b->stream));          // all-zero again: the next launch's precondition (nobody waits for it here)
    b->gtable_dirty = false;
  }
  L->t1 = std::chrono::steady_clock::now();
  L->launched = true;
  return PG_OK;
}

pg_status finish_group_launch(DeferredLaunch* L, std::vector<Deferred>& defs, pg_result* results, pg_status* statuses) {
  BatchCtx* b = L->b;
  const int n = L->n;
  static const bool trace = getenv("PINOT_GPU_BATCH_TRACE") != nullptr;
  HIP_TRY(hipSetDevice(phys_device(L->device)));
  float ms = 0.f;
  if (L->publish) {
    // Every item's last workgroup has written the item's slice to the pinned image and then the launch's sequence number to the item's
    // record: an item is converted as soon as ITS number is there.  The items of a launch run side by side (every item has its share of the
    // resident workgroups), so their numbers arrive together near the end of the kernel -- measured (profiles/r6/group_publish_trace.txt): what
    // this form saves is the copy command and the memset behind the kernel (~70 us at 64 x 1 000 groups) and the helpers' wake-up (they are
    // woken when the kernel starts, sleep through most of its expected duration and poll the rest: ~12 us of conversion per item then
    // starts the moment the numbers are there).
    const unsigned long long seq = L->seq;
    const int conv_threads = n <= 1 ? 1 : (int)std::max(1u, std::min(32u, std::thread::hardware_concurrency() / 2));      // (64 threads, one round of conversions, measured slower: 0.72-0.75 ms against 0.69-0.70)
    // (a group-by streams at most ~1.1 G docs per ms: 60 % of that time is slept, not polled, when it is worth a sleep)
    const auto sleep_until = L->t1 + std::chrono::nanoseconds((long long)((double)L->docs / 1100.0 * 0.6));
    const bool sleep_first = n > 1 && (double)L->docs / 1100.0 * 0.6 > 200'000.0;      // (nanoseconds)
    std::atomic<int> unpublished{0};
    std::atomic<long long> convert_ns{0}, wait_ns{0};          // (PINOT_GPU_BATCH_TRACE: summed over the items)
    run_items(n, conv_threads, 1, false, [&](int k) {
      const int i = L->items[(size_t)k];
      volatile unsigned long long* const flag = &b->h_records[k].seq;
      if (sleep_first && *flag != seq && std::chrono::steady_clock::now() < sleep_until) std::this_thread::sleep_until(sleep_until);
      const auto tw0 = trace ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
      (void)wait_polled(b->stream, L->docs, [&] { return *flag == seq; });
      const auto tw1 = trace ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
      if (*flag != seq) { unpublished.fetch_add(1); statuses[i] = fail(PG_ERR_INTERNAL, "batch item %d did not publish its group table", i); return; }
      defs[(size_t)i].item->convert_group(b->h_gtable + L->table_offsets[(size_t)k], &results[i]);
      statuses[i] = PG_OK;
      if (trace) { wait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(tw1 - tw0).count(); convert_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tw1).count(); }
    });
    if (unpublished.load() != 0) b->gtable_dirty = true;
    if (L->timed) { HIP_TRY(hipEventSynchronize(b->ev[1])); HIP_TRY(hipEventElapsedTime(&ms, b->ev[0], b->ev[1])); }
    for (int k = 0; k < n; ++k) {
      const int i = L->items[(size_t)k];
      if (statuses[i] != PG_OK) continue;
      const float share = L->total_blocks > 0 ? ms * (float)L->blocks[(size_t)k] / (float)L->total_blocks : 0.f;
      results[i].device_ms = share;
      results[i].dominant_kernel_ms = share;
    }
    if (trace) fprintf(stderr, "  deferred group-by launch on device %d: %d items %lld workgroups, lds %zu, enqueue %.1f us, items published and converted %.1f us behind it (waits %.1f us, conversions %.1f us summed over the items), kernel %.1f us\n", L->device, n,
                       L->total_blocks, L->lds, std::chrono::duration<double, std::micro>(L->t1 - L->t0).count(), std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - L->t1).count(),
                       (double)wait_ns.load() * 1e-3, (double)convert_ns.load() * 1e-3, ms * 1e3);
    return PG_OK;
  }
  HIP_TRY(hipEventSynchronize(b->ev[2]));
  const auto t2 = std::chrono::steady_clock::now();
  if (L->timed) HIP_TRY(hipEventElapsedTime(&ms, b->ev[0], b->ev[1]));
  // the items' conversions (a thousand groups each: ~10 us) side by side on the library's worker threads
  run_items(n, (int)std::max(1u, std::min(32u, std::thread::hardware_concurrency() / 2)), 1, false, [&](int k) {
    const int i = L->items[(size_t)k];
    defs[(size_t)i].item->convert_group(b->h_gtable + L->table_offsets[(size_t)k], &results[i]);
    const float share = L->total_blocks > 0 ? ms * (float)L->blocks[(size_t)k] / (float)L->total_blocks : 0.f;
    results[i].device_ms = share;
    results[i].dominant_kernel_ms = share;
    statuses[i] = PG_OK;
  });
  if (trace) fprintf(stderr, "  deferred group-by launch on device %d: %d items %lld workgroups, lds %zu, enqueue %.1f us, wait %.1f us, kernel %.1f us, convert %.1f us\n", L->device, n, L->total_blocks, L->lds,
                     std::chrono::duration<double, std::micro>(L->t1 - L->t0).count(), std::chrono::duration<double, std::micro>(t2 - L->t1).count(), ms * 1e3,
                     std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t2).count());
  return PG_OK;
}

// The index-led items of one device (BatchKind::IndexAnd): one launch of index_and_batch_kernel -- the items' workgroups
// in proportion to their windows, about what is resident in total -- every item with its own records, arrival counters and pinned host record.
static_assert(sizeof(IndexAndParams) <= kBatchItemSlot, "an index-AND item takes a slot of the batch's parameter blob");
pg_status enqueue_index_and_launch(DeferredLaunch* L, BatchCtx* b, std::vector<Deferred>& defs, pg_segment* const* segments) {
  const std::vector<int>& items = L->items;
  const int n = L->n;
  long long total_windows = 0;
  for (int i : items) { total_windows += defs[(size_t)i].item->and_windows; L->docs += (long long)segments[i]->num_docs; }
  const long long budget = (long long)segments[items[0]]->num_cus * index_and_batch_blocks_per_cu();      // workgroups (of index_and_batch_block_waves() wavefronts) resident at once
  std::vector<int>& blocks = L->blocks;
  blocks.assign((size_t)n, 0);
  size_t partials = 0;
  long long total_blocks = 0;
  for (int k = 0; k < n; ++k) {
    const LoweredItem& d = *defs[(size_t)items[(size_t)k]].item;
    const long long share = total_windows > 0 ? ((long long)d.and_windows * budget + total_windows - 1) / total_windows : 1;
    blocks[(size_t)k] = (int)std::max<long long>(1, std::min<long long>((long long)d.blocks, share));
    partials += (size_t)blocks[(size_t)k] + (size_t)kFoldExtraRecords;
    total_blocks += blocks[(size_t)k];
  }
  L->total_blocks = total_blocks;
  pg_status st = ensure_batch_ctx(b, n, partials);
  if (st != PG_OK) return st;
  IndexAndParams* h_items = reinterpret_cast<IndexAndParams*>(b->h_blob + b->items_offset);
  const IndexAndParams* d_items = reinterpret_cast<const IndexAndParams*>(b->d_blob + b->items_offset);
  size_t off = 0;
  uint32_t first = 0;
  const unsigned long long seq = L->seq = ++b->seq;
  for (int k = 0; k < n; ++k) {
    const LoweredItem& d = *defs[(size_t)items[(size_t)k]].item;
    IndexAndParams& ap = h_items[k];               // (the pinned copy the device reads: filled in place)
    ap = *d.and_params;
    ap.num_windows = (int32_t)d.and_windows;
    ap.out = nullptr; ap.window_info = nullptr;     // record mode: neither a bitmap nor window masks
    ap.shards = nullptr;
    memset(&ap.pub, 0, sizeof(ap.pub));
    ap.pub.done_counter = b->d_done + (size_t)k * (kFoldShards + 1) * kFoldStride;
    ap.pub.partials = b->d_partials + off;
    off += (size_t)blocks[(size_t)k] + (size_t)kFoldExtraRecords;
    ap.pub.host_out = b->h_records_dev + k;
    ap.pub.host_seq = seq;
    ap.pub.fold_slots = ap.gather_cols;
    ap.pub.fold_one_counter = g_engine.fold_one_counter;
    b->h_first[k] = first;
    first += (uint32_t)blocks[(size_t)k];
  }
  b->h_first[n] = first;
  L->timed = (g_engine.flags & PG_CFG_TIME_KERNELS) != 0;
  L->t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipMemcpyAsync(b->d_blob, b->h_blob, b->items_offset + sizeof(IndexAndParams) * (size_t)n, hipMemcpyHostToDevice, b->stream));
  if (L->timed) HIP_TRY(hipEventRecord(b->ev[0], b->stream));
  launch_index_and_batch((int)total_blocks, b->stream, d_items, b->d_first, n);
  HIP_TRY(hipGetLastError());
  if (L->timed) HIP_TRY(hipEventRecord(b->ev[1], b->stream));
  L->t1 = std::chrono::steady_clock::now();
  L->launched = true;
  return PG_OK;
}

pg_status enqueue_deferred(DeferredLaunch* L, std::vector<Deferred>& defs, pg_segment* const* segments) {
  const int device = L->device;
  const std::vector<int>& items = L->items;
  HIP_TRY(hipSetDevice(phys_device(device)));
  BatchCtx* b = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_batch_mu);
    // The context released LAST is taken first (round 6b).  Taken from the front, a caller rotated through every context the process had ever
    // needed at once -- sixteen after sixteen threads had run group-bys side by side -- and each of them grew its blob, set area and group
    // table on ITS first use by the new shape: the first dozen calls of a shape took twice their time (PINOT_GPU_BATCH_TRACE,
    // profiles/r6/batch_ctx_pool_lifo.txt; DESIGN.md section 9's "C5x64 in a busy process").
    for (size_t i = g_batch_free.size(); i-- > 0;) if (g_batch_free[i]->device == device) { b = g_batch_free[i]; g_batch_free.erase(g_batch_free.begin() + (long)i); break; }
  }
  if (!b) { b = new BatchCtx(); b->device = device; }
  L->b = b;
  const int n = L->n = (int)items.size();
  if (L->kind == BatchKind::GroupLds) return enqueue_group_launch(L, b, defs, segments);
  if (L->kind == BatchKind::IndexAnd) return enqueue_index_and_launch(L, b, defs, segments);
  // Workgroups per item in proportion to its tiles, about sixteen per CU in total (four waves each: ~4x what is resident, so that
  // the items' tails overlap other items' scans); never more than the item would get on its own.
  long long total_tiles = 0;
  for (int i : items) { total_tiles += doc_tiles(segments[i]); L->docs += (long long)segments[i]->num_docs; }
  // (the lean kernels hold five -- raw: four -- waves per SIMD: a workgroup per CU more than the general body's four)
  const BatchKindInfo info = batch_kind_info(L->kind);
  const int wpb = info.block_waves, tiles_per_wave = info.tiles_per_wave;
  size_t launch_lds = 0;
  for (int i : items) launch_lds = std::max(launch_lds, defs[(size_t)i].item->hist_lds);
  L->lds = launch_lds;
  int lean_bpc = std::max(1, info.wave_cap / wpb);
  if (info.hist_bits) lean_bpc = std::max(1, std::min(info.wave_cap / wpb, (int)((160 * 1024 - 2048) / (launch_lds + 256))));
  const bool bpc_forced = g_engine.batch_blocks_per_cu_forced;      // (read once per pg_init: bench sweeps re-initialise the engine with it)
  const bool lean = L->kind != BatchKind::Private && (!bpc_forced || info.hist_bits != 0);
  const long long budget = (long long)segments[items[0]]->num_cus * (lean ? lean_bpc : g_engine.batch_blocks_per_cu);
  const std::vector<int>& blocks = L->blocks;
  const long long total_blocks = share_blocks(L, defs, segments, total_tiles, budget, (long long)wpb * tiles_per_wave);
  size_t partials = 0;
  bool one_slot = true;
  for (int k = 0; k < n; ++k) { partials += (size_t)blocks[(size_t)k] + (size_t)kFoldExtraRecords; one_slot = one_slot && defs[(size_t)items[(size_t)k]].item->one_slot; }
  size_t set_bytes = 0;
  for (int i : items) set_bytes += item_set_bytes(*defs[(size_t)i].item);
  pg_status st = ensure_batch_ctx(b, n, partials, set_bytes);
  if (st != PG_OK) return st;
  size_t off = 0, set_off = 0;
  uint32_t first = 0;
  const unsigned long long seq = L->seq = ++b->seq;
  for (int k = 0; k < n; ++k) {
    ScanParams& sp = b->h_items[k];               // (the pinned copy the device reads: filled in place)
    sp = defs[(size_t)items[(size_t)k]].item->sp;
    place_item_sets(b, *defs[(size_t)items[(size_t)k]].item, &sp, &set_off);
    sp.partials = b->d_partials + off;
    off += (size_t)blocks[(size_t)k] + (size_t)kFoldExtraRecords;
    sp.done_counter = b->d_done + (size_t)k * (kFoldShards + 1) * kFoldStride;
    sp.host_out = b->h_records_dev + k;
    sp.host_seq = seq;
    b->h_first[k] = first;
    first += (uint32_t)blocks[(size_t)k];
  }
  b->h_first[n] = first;
  L->timed = (g_engine.flags & PG_CFG_TIME_KERNELS) != 0;
  L->t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipMemcpyAsync(b->d_blob, b->h_blob, b->items_offset + sizeof(ScanParams) * (size_t)n, hipMemcpyHostToDevice, b->stream));
  if (set_off) HIP_TRY(hipMemcpyAsync(b->d_blob + b->sets_offset, b->h_blob + b->sets_offset, set_off, hipMemcpyHostToDevice, b->stream));
  if (L->timed) HIP_TRY(hipEventRecord(b->ev[0], b->stream));
  launch_batch_kind(L->kind, info, one_slot, (int)total_blocks, launch_lds, b->stream, b->d_items, b->d_first, n);
  HIP_TRY(hipGetLastError());
  if (L->timed) HIP_TRY(hipEventRecord(b->ev[1], b->stream));
  L->t1 = std::chrono::steady_clock::now();
  L->launched = true;
  return PG_OK;
}

pg_status finish_deferred(DeferredLaunch* L, std::vector<Deferred>& defs, pg_result* results, pg_status* statuses) {
  if (L->kind == BatchKind::GroupLds) return finish_group_launch(L, defs, results, statuses);
  BatchCtx* b = L->b;
  const int n = L->n;
  const unsigned long long seq = L->seq;
  static const bool trace = getenv("PINOT_GPU_BATCH_TRACE") != nullptr;
  HIP_TRY(hipSetDevice(phys_device(L->device)));
  if (g_engine.poll_result && !L->timed) {
    // every item publishes its own pinned record: their sequence numbers are the completion signal (as in pg_execute)
    int k = 0;
    const pg_status st = wait_polled(b->stream, L->docs, [&] { while (k < n && *(volatile unsigned long long*)&b->h_records[k].seq == seq) ++k; return k == n; });
    if (st != PG_OK) return st;
  } else {
    HIP_TRY(hipStreamSynchronize(b->stream));
  }
  const auto t2 = std::chrono::steady_clock::now();
  float ms = 0.f;
  if (L->timed) HIP_TRY(hipEventElapsedTime(&ms, b->ev[0], b->ev[1]));
  if (trace) fprintf(stderr, "  deferred launch on device %d: %d items %lld workgroups, sizeof(ScanParams) %zu, enqueue %.1f us, wait %.1f us, kernel %.1f us\n", L->device, n, L->total_blocks,
                     sizeof(ScanParams), std::chrono::duration<double, std::micro>(L->t1 - L->t0).count(), std::chrono::duration<double, std::micro>(t2 - L->t1).count(), ms * 1e3);
  for (int k = 0; k < n; ++k) {
    const int i = L->items[(size_t)k];
    if (b->h_records[k].seq != seq) { statuses[i] = fail(PG_ERR_INTERNAL, "batch item %d did not publish its record", i); continue; }
    if (b->h_records[k].partial.flags & kPartialStale) { statuses[i] = fail(PG_ERR_INTERNAL, "batch item %d: the fold read a record that was not written by this launch", i); continue; }
    const LoweredItem& it = *defs[(size_t)i].item;
    if (it.hist_cw != 0 && it.hist_cw < 32 && (unsigned long long)b->h_records[k].partial.sum[1] != b->h_records[k].partial.count) {
      // a plain narrow counter wrapped (skewed dictIds): the histogram's sum is not used -- pg_execute answers this item again and moves
      // the column to the guarded tier, where its items run launches of their own (scan_hist_kernel's header: exact or not used)
      statuses[i] = kRunAlone;
      continue;
    }
    defs[(size_t)i].item->convert(b->h_records[k].partial, &results[i]);
    // ONE launch serves all items of the device: each item is charged its share of the workgroups, so that summing device_ms over a
    // batch's results gives the launch's time once (pg_result.device_ms of a batch item is an apportioned figure, not a measurement of its own)
    const float share = L->total_blocks > 0 ? ms * (float)L->blocks[(size_t)k] / (float)L->total_blocks : 0.f;
    results[i].device_ms = share;
    results[i].dominant_kernel_ms = share;
    statuses[i] = PG_OK;
  }
  return PG_OK;
}

}  // namespace

// A group-by of the LDS-table form (key space up to the LDS table: the C3 shape) is ONE launch here too: the one-item form of the batch's
// group_lds_batch_kernel -- no init_group_table_kernel, no count / scan / compact launches and the two waits between them; the item's
// all-zero table slice comes back whole and the host keeps the slots whose count is not zero (§4.1k).  Its lowering is remembered in the
// segment's plan cache like a batch item's.  Everything else takes execute_one as before.  PINOT_GPU_GROUP_ONE_LAUNCH=0: never.
pg_status pg_execute(pg_segment* segment, const pg_query* query, pg_result* out_result) {
  if (reserved_flags(query)) { if (out_result) memset(out_result, 0, sizeof(*out_result)); return fail_reserved_flags(query); }
  if (const pg_aggregation* bad = bad_function_word(query)) { if (out_result) memset(out_result, 0, sizeof(*out_result)); return fail_function_word(bad); }
  if (has_moments(query)) return execute_moments(segment, query, out_result);
  if (has_percentile(query)) return execute_percentile(segment, query, out_result);
  if (has_distinct(query)) return execute_distinct(segment, query, out_result);
  // (PG_CFG_PROFILE_WAVES: the per-wave phase counters live in the kernels execute_one launches itself, and its HIP events bracket ALL of a
  //  query's launches -- the deferred form would leave profile_* empty and report the kernel bracket only)
  if (!(g_engine.group_one_launch && g_engine.batch_launch && g_engine.batch_group && segment && query && out_result && query->num_group_by > 0 &&
        !(query->flags & PG_QUERY_NULL_HANDLING) && !(g_engine.flags & PG_CFG_PROFILE_WAVES) && g_engine.initialized))
  {
    if (exec_trace_on()) { memset(t_exec_trace.seen, 0, sizeof(t_exec_trace.seen)); exec_mark(0); }
    const pg_status st = execute_one(segment, query, out_result, nullptr);
    if (exec_trace_on()) {
      exec_mark(5);
      const ExecTrace& x = t_exec_trace;
      auto us = [&](int a, int b) { return (x.seen[a] && x.seen[b]) ? std::chrono::duration<double, std::micro>(x.t[b] - x.t[a]).count() : -1.0; };
      fprintf(stderr, "exec trace: status %d, check %.1f us, context + lowering %.1f us, launches %.1f us, wait %.1f us, after the wait %.1f us, total %.1f us (-1: phase not passed)\n",
              (int)st, us(0, 1), us(1, 2), us(2, 3), us(3, 4), us(4, 5), us(0, 5));
    }
    return st;
  }
  std::vector<Deferred> defs(1);
  defs[0].single = true;
  std::string key;
  pg_status st = kDeferred;
  const bool keyed = g_engine.plan_cache && query_key(query, &key);
  if (keyed && cached_item(segment, key, &defs[0]) && defs[0].item->gp != nullptr) {
    memset(out_result, 0, sizeof(*out_result));
  } else {
    defs[0] = Deferred();
    defs[0].single = true;
    std::shared_ptr<const OwnedQuery> copy;
    const pg_query* q = query;
    if (keyed && !key.empty()) { copy = own_query(query); q = &copy->q; }
    st = execute_one(segment, q, out_result, &defs[0]);
    if (st == kDeferred && copy && defs[0].cacheable) remember_item(segment, std::move(key), copy, &defs[0]);
    else if (st == kDeferred && copy) std::const_pointer_cast<LoweredItem>(defs[0].item)->query = copy;
    if (st != kDeferred) return st;                     // ran the usual way (or failed): nothing was deferred
  }
  DeferredLaunch L;
  L.device = segment->device; L.kind = BatchKind::GroupLds; L.items.push_back(0);
  pg_segment* const segs[1] = {segment};
  pg_status item_status = PG_ERR_INTERNAL;
  st = enqueue_deferred(&L, defs, segs);
  if (st == PG_OK) st = finish_deferred(&L, defs, out_result, &item_status);
  if (st == PG_OK) st = item_status;
  if (st != PG_OK) pg_result_free(out_result);
  return st;
}

pg_status pg_execute_batch(pg_segment* const* segments, const pg_query* const* queries, int32_t count, pg_result* results, pg_status* statuses) {
  if (!g_engine.initialized) return fail(PG_ERR_NOT_INITIALIZED, "pg_init has not been called");
  if (count < 0 || (count > 0 && (!segments || !queries || !results || !statuses))) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  for (int i = 0; i < count; ++i) { memset(&results[i], 0, sizeof(pg_result)); statuses[i] = PG_ERR_INVALID_ARGUMENT; }
  if (count == 0) return PG_OK;
  static const bool trace = getenv("PINOT_GPU_BATCH_TRACE") != nullptr;      // host phases of every call on stderr
  const auto t_begin = std::chrono::steady_clock::now();
  std::vector<Deferred> defs((size_t)count);
  std::vector<std::string> errors((size_t)count);
  // 1. every item is lowered (and, when it cannot share the launch, run on a context of its own) on the library's worker threads --
  // except the items whose segment has this very query in its plan cache: those are picked up on the calling thread (~0.2 us each)
  const int threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency() / 2));
  std::vector<float> item_us(trace ? (size_t)count : 0);
  const bool plan_cache = g_engine.plan_cache;
  std::vector<int> todo;
  std::vector<std::string> keys(plan_cache && g_engine.batch_launch ? (size_t)count : 0);
  int cache_hits = 0;
  for (int i = 0; i < count; ++i) {
    if (!keys.empty() && segments[i] && queries[i] && !(queries[i]->flags & PG_QUERY_NULL_HANDLING) && query_key(queries[i], &keys[(size_t)i]) &&
        cached_item(segments[i], keys[(size_t)i], &defs[(size_t)i])) { statuses[i] = kDeferred; ++cache_hits; continue; }
    todo.push_back(i);
  }
  // (a deferred item is ~2 us of lowering: eight per claim, so 64 items wake at most seven helpers; an item that runs its own kernel
  // is claimed alone)
  // (an item too large for the shared launch runs its whole kernel inside its claim: such batches are claimed one item at a time)
  bool all_small = g_engine.batch_launch;
  for (int i : todo) all_small = all_small && segments[i] != nullptr && doc_tiles(segments[i]) <= kBatchMaxTiles;
  const int todo_count = (int)todo.size();
  if (todo_count > 0) run_items(todo_count, all_small ? threads : std::min(threads, todo_count), all_small ? 8 : 1, !all_small, [&](int t) {
    const int i = todo[(size_t)t];
    if (!segments[i] || !queries[i]) { statuses[i] = PG_ERR_INVALID_ARGUMENT; errors[(size_t)i] = "null segment or query"; return; }
    if (reserved_flags(queries[i])) { statuses[i] = fail_reserved_flags(queries[i]); errors[(size_t)i] = g_error; return; }
    if (const pg_aggregation* bad = bad_function_word(queries[i])) { statuses[i] = fail_function_word(bad); errors[(size_t)i] = g_error; return; }
    const auto t_item = trace ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
    // (a query that may enter the plan cache is lowered from a copy of its own: the item's conversion reads the query after this call has returned)
    const pg_query* q = queries[i];
    std::shared_ptr<const OwnedQuery> copy;
    if (!keys.empty() && !keys[(size_t)i].empty()) { copy = own_query(q); q = &copy->q; }
    // (a DISTINCTCOUNT / PERCENTILE / VARIANCE item runs as a pg_execute of its own: no shared launch)
    statuses[i] = has_moments(q) ? execute_moments(segments[i], q, &results[i]) : has_percentile(q) ? execute_percentile(segments[i], q, &results[i]) : has_distinct(q) ? execute_distinct(segments[i], q, &results[i]) : execute_one(segments[i], q, &results[i], g_engine.batch_launch ? &defs[(size_t)i] : nullptr);
    if (statuses[i] == kDeferred && copy && defs[(size_t)i].cacheable) remember_item(segments[i], std::move(keys[(size_t)i]), copy, &defs[(size_t)i]);
    else if (statuses[i] == kDeferred && copy) std::const_pointer_cast<LoweredItem>(defs[(size_t)i].item)->query = copy;
    if (trace) item_us[(size_t)i] = std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - t_item).count();
    if (statuses[i] != PG_OK && statuses[i] != kDeferred) errors[(size_t)i] = g_error;      // (g_error is the worker's thread-local)
  });
  const auto t_lowered = std::chrono::steady_clock::now();
  // 2. the deferred items, one launch per device: every device's launch is enqueued before any of them is waited for
  std::vector<std::unique_ptr<DeferredLaunch>> launches;
  for (int i = 0; i < count; ++i) {
    if (statuses[i] != kDeferred) continue;
    DeferredLaunch* L = nullptr;
    const BatchKind kind = static_cast<BatchKind>(defs[(size_t)i].item->sp.lean_kind);
    for (auto& l : launches) if (l->device == segments[i]->device && l->kind == kind) L = l.get();
    if (!L) { launches.emplace_back(new DeferredLaunch()); L = launches.back().get(); L->device = segments[i]->device; L->kind = kind; }
    L->items.push_back(i);
  }
  auto fail_items = [&](DeferredLaunch* L, pg_status st) {
    for (int i : L->items) if (statuses[i] == kDeferred) { statuses[i] = st; errors[(size_t)i] = g_error; pg_result_free(&results[i]); }
  };
  for (auto& l : launches) { const pg_status st = enqueue_deferred(l.get(), defs, segments); if (st != PG_OK) fail_items(l.get(), st); }
  for (auto& l : launches) {
    if (!l->launched) continue;
    const pg_status st = finish_deferred(l.get(), defs, results, statuses);
    if (st != PG_OK) fail_items(l.get(), st);
    else for (int i : l->items) if (statuses[i] != PG_OK) errors[(size_t)i] = g_error;
  }
  for (int i = 0; i < count; ++i) {
    if (statuses[i] != kRunAlone) continue;
    defs[(size_t)i].planes.reset();
    statuses[i] = execute_one(segments[i], queries[i], &results[i], nullptr);
    if (statuses[i] != PG_OK) errors[(size_t)i] = g_error;
  }
  // pg_last_error of the caller: the first failed item's message
  for (int i = 0; i < count; ++i) if (statuses[i] != PG_OK) { g_error = "batch item " + std::to_string(i) + ": " + errors[(size_t)i]; break; }
  if (trace) {
    const auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    float sum_us = 0.f, max_us = 0.f;
    for (float v : item_us) { sum_us += v; max_us = std::max(max_us, v); }
    fprintf(stderr, "pg_execute_batch: %d items (%d from the plan cache), lower %.1f us (items: sum %.1f us, max %.1f us, %d threads), launches %.1f us\n", count, cache_hits,
            us(t_begin, t_lowered), sum_us, max_us, threads, us(t_lowered, std::chrono::steady_clock::now()));
  }
  return PG_OK;
}

pg_status pg_segment_plane_bytes(const pg_segment* segment, uint64_t* out_bytes) {
  if (!segment || !out_bytes) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  std::lock_guard<std::mutex> lk(g_planes.mu);
  *out_bytes = segment->plane_bytes;
  return PG_OK;
}

pg_status pg_set_plane_budget(uint64_t budget_bytes, uint64_t* out_previous) {
  std::lock_guard<std::mutex> lk(g_planes.mu);
  if (out_previous) *out_previous = g_planes.budget_bytes;
  g_planes.budget_bytes = budget_bytes;
  return PG_OK;
}

// ---- doc sets (include/pinot_gpu.h): the queryable docIds of an upsert / dedup segment ----
static std::atomic<int64_t> g_next_doc_set_id{1};      // unique for the life of the process: an id that was released never names another set

// The largest docId a parsed container holds (its payload lies inside the buffer: parse_roaring checked).
static uint32_t container_last_doc(const uint8_t* data, const DevContainer& dc) {
  const uint8_t* p = data + dc.offset;
  uint32_t low = 0;
  if (dc.type == 0) low = le16(p + 2ull * (dc.cardinality - 1));
  else if (dc.type == 1) { for (int b = 8191; b >= 0; --b) if (p[b]) { low = (uint32_t)b * 8u + (31u - (uint32_t)__builtin_clz((unsigned)p[b])); break; } }
  else if (dc.num_runs > 0) low = (uint32_t)le16(p + 2 + 4ull * (dc.num_runs - 1)) + (uint32_t)le16(p + 4 + 4ull * (dc.num_runs - 1));
  return (dc.key << 16) + low;
}

pg_status pg_doc_set_create(pg_segment* segment, int32_t format, const void* data, uint64_t size, int64_t* out_id) {
  if (!g_engine.initialized) return fail(PG_ERR_NOT_INITIALIZED, "pg_init has not been called");
  if (!segment || !out_id || (size > 0 && !data)) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  if (format != PG_DOC_SET_ROARING && format != PG_DOC_SET_WORDS) return fail(PG_ERR_INVALID_ARGUMENT, "unknown doc set format %d", format);
  const long long padded_words = (long long)std::max(segment->num_tiles, 1) * kMaxTileSteps;
  const size_t doc_words = ((size_t)segment->num_docs + 63) / 64;
  auto ds = std::make_shared<DocSet>();
  ds->bytes = (uint64_t)padded_words * 8;
  std::vector<DevContainer> kept;
  if (format == PG_DOC_SET_WORDS) {
    if (size != (uint64_t)doc_words * 8) return fail(PG_ERR_INVALID_ARGUMENT, "doc set: %llu bytes of words for %d docs (expected %zu)", (unsigned long long)size, segment->num_docs, doc_words * 8);
    const uint8_t* bytes = (const uint8_t*)data;
    for (size_t w = 0; w < doc_words; ++w) { uint64_t v; memcpy(&v, bytes + 8 * w, 8); ds->cardinality += __builtin_popcountll(v); }
    if (doc_words > 0 && (segment->num_docs & 63)) {
      uint64_t last; memcpy(&last, bytes + 8 * (doc_words - 1), 8);
      if (last >> (segment->num_docs & 63)) return fail(PG_ERR_INVALID_ARGUMENT, "doc set: a bit beyond numDocs (%d) is set", segment->num_docs);
    }
  } else {
    std::vector<DevContainer> dir;
    const pg_status pst = parse_roaring((const uint8_t*)data, 0, size, &dir);
    if (pst != PG_OK) return pst;
    for (const DevContainer& dc : dir) {
      if (dc.type == 2 && dc.num_runs == 0) continue;
      if (segment->num_docs <= 0 || (dc.key << 16) >= (uint32_t)segment->num_docs || container_last_doc((const uint8_t*)data, dc) >= (uint32_t)segment->num_docs)
        return fail(PG_ERR_INVALID_ARGUMENT, "doc set: a docId of container %u is beyond numDocs (%d)", dc.key, segment->num_docs);
      kept.push_back(dc);
      ds->cardinality += dc.cardinality;
    }
  }
  HIP_TRY(hipSetDevice(phys_device(segment->device)));
  hipError_t e = hipMalloc((void**)&ds->d_words, (size_t)ds->bytes);
  if (e != hipSuccess) { (void)hipGetLastError(); ds->d_words = nullptr; return fail(PG_ERR_OUT_OF_MEMORY, "doc set: hipMalloc(%llu): %s", (unsigned long long)ds->bytes, hipGetErrorString(e)); }
  e = hipMemset(ds->d_words, 0, (size_t)ds->bytes);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // (a large upload below runs on the staging pool's own streams: the zeros are there first)
  if (format == PG_DOC_SET_WORDS) {
    if (e == hipSuccess && size > 0) e = h2d_copy(ds->d_words, data, (size_t)size, phys_device(segment->device));
  } else if (!kept.empty()) {
    // the serialized bitmap and its container directory go up, roaring_expand_kernel writes the doc-order words (one 65536-doc window per workgroup)
    uint8_t* d_bytes = nullptr;
    DevContainer* d_cont = nullptr;
    if (e == hipSuccess) e = hipMalloc((void**)&d_bytes, (size_t)size + 64);
    if (e == hipSuccess) e = h2d_copy(d_bytes, data, (size_t)size, phys_device(segment->device));
    if (e == hipSuccess) e = hipMalloc((void**)&d_cont, kept.size() * sizeof(DevContainer));
    if (e == hipSuccess) e = hipMemcpy(d_cont, kept.data(), kept.size() * sizeof(DevContainer), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      roaring_expand_kernel<<<dim3((unsigned)((padded_words + 1023) / 1024)), dim3(kBlockThreads), 0, 0>>>(d_bytes, d_cont, 0, (int)kept.size(), ds->d_words, padded_words, 0);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (d_bytes) (void)hipFree(d_bytes);
    if (d_cont) (void)hipFree(d_cont);
  }
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(PG_ERR_DEVICE, "doc set upload: %s", hipGetErrorString(e)); }
  ds->id = g_next_doc_set_id.fetch_add(1);
  segment->device_bytes += ds->bytes;
  *out_id = ds->id;
  std::lock_guard<std::mutex> lk(segment->doc_sets_mu);
  segment->doc_sets.push_back(std::move(ds));
  return PG_OK;
}

pg_status pg_doc_set_release(pg_segment* segment, int64_t id) {
  if (!g_engine.initialized) return fail(PG_ERR_NOT_INITIALIZED, "pg_init has not been called");
  if (!segment) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  std::shared_ptr<DocSet> ds;
  {
    std::lock_guard<std::mutex> lk(segment->doc_sets_mu);
    for (size_t i = 0; i < segment->doc_sets.size(); ++i) if (segment->doc_sets[i]->id == id) { ds = std::move(segment->doc_sets[i]); segment->doc_sets.erase(segment->doc_sets.begin() + (long)i); break; }
  }
  if (!ds) return fail(PG_ERR_INVALID_ARGUMENT, "doc set %lld is unknown to segment %s (never created, or released)", (long long)id, segment->name.c_str());
  segment->device_bytes -= ds->bytes;
  // lowerings the segment remembers must not outlive the caller's reference: a later query with this id is refused, not served from the cache
  std::lock_guard<std::mutex> lk(segment->plan_cache_mu);
  auto& cache = segment->plan_cache;
  cache.erase(std::remove_if(cache.begin(), cache.end(), [&](const std::shared_ptr<const LoweredItem>& it) {
    for (const auto& held : it->doc_sets) if (held->id == id) return true;
    return false;
  }), cache.end());
  return PG_OK;      // (the bitmap itself goes when the last query that reads it has finished: ~DocSet)
}

pg_status pg_doc_set_cardinality(const pg_segment* segment, int64_t id, int64_t* out_cardinality) {
  if (!g_engine.initialized) return fail(PG_ERR_NOT_INITIALIZED, "pg_init has not been called");
  if (!segment || !out_cardinality) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  const std::shared_ptr<DocSet> ds = find_doc_set(segment, id);
  if (!ds) return fail(PG_ERR_INVALID_ARGUMENT, "doc set %lld is unknown to segment %s (never created, or released)", (long long)id, segment->name.c_str());
  *out_cardinality = ds->cardinality;
  return PG_OK;
}

pg_status pg_query_check(const pg_segment* segment, const pg_query* query) {
  if (!g_engine.initialized) return fail(PG_ERR_NOT_INITIALIZED, "pg_init has not been called");
  if (!segment || !query) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  if (reserved_flags(query)) return fail_reserved_flags(query);
  if (const pg_aggregation* bad = bad_function_word(query)) return fail_function_word(bad);
  if (has_moments(query)) { MomentsPlan plan; return plan_moments(segment, query, &plan); }
  if (has_percentile(query)) { PercentilePlan plan; return plan_percentile(segment, query, &plan); }
  if (has_distinct(query)) { DistinctPlan plan; return plan_distinct(segment, query, &plan); }
  return check_ordinary_query(segment, query);
}

pg_status pg_result_distinct_dict_ids(const pg_result* result, int32_t aggregation, int32_t group_row, const uint32_t** out_words, int32_t* out_num_words) {
  if (!result || !out_words || !out_num_words) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  *out_words = nullptr; *out_num_words = 0;
  const ResultInternal* sets = static_cast<const ResultInternal*>(result->internal);
  if (aggregation < 0 || aggregation >= result->num_aggregations) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation %d out of range", aggregation);
  const DistinctSet* ds = nullptr;
  if (sets) for (const DistinctSet& s : sets->distinct) if (s.aggregation == aggregation) ds = &s;
  if (!ds) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation %d is not a PG_AGG_DISTINCTCOUNT", aggregation);
  const bool grouped = result->group_aggregations != nullptr;
  if (grouped ? (group_row < 0 || group_row >= result->num_groups || group_row >= ds->rows) : group_row != -1)
    return fail(PG_ERR_INVALID_ARGUMENT, "group row %d out of range", group_row);
  *out_words = ds->words.data() + (size_t)(grouped ? group_row : 0) * (size_t)ds->num_words;
  *out_num_words = ds->num_words;
  return PG_OK;
}

pg_status pg_result_hll_registers(const pg_result* result, int32_t aggregation, int32_t group_row, const uint8_t** out_registers, int32_t* out_num_registers) {
  if (!result || !out_registers || !out_num_registers) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  *out_registers = nullptr; *out_num_registers = 0;
  const ResultInternal* sets = static_cast<const ResultInternal*>(result->internal);
  if (aggregation < 0 || aggregation >= result->num_aggregations) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation %d out of range", aggregation);
  const HllSet* hs = nullptr;
  if (sets) for (const HllSet& s : sets->hll) if (s.aggregation == aggregation) hs = &s;
  if (!hs) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation %d is not a PG_AGG_DISTINCTCOUNTHLL", aggregation);
  const bool grouped = result->group_aggregations != nullptr;
  if (grouped ? (group_row < 0 || group_row >= result->num_groups || group_row >= hs->rows) : group_row != -1)
    return fail(PG_ERR_INVALID_ARGUMENT, "group row %d out of range", group_row);
  *out_registers = hs->registers.data() + ((size_t)(grouped ? group_row : 0) << hs->log2m);
  *out_num_registers = 1 << hs->log2m;
  return PG_OK;
}

pg_status pg_result_moments(const pg_result* result, int32_t aggregation, int32_t group_row, int64_t* out_count, double* out_sum, double* out_m2) {
  if (!result || !out_count || !out_sum || !out_m2) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  *out_count = 0; *out_sum = 0.0; *out_m2 = 0.0;
  const ResultInternal* sets = static_cast<const ResultInternal*>(result->internal);
  if (aggregation < 0 || aggregation >= result->num_aggregations) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation %d out of range", aggregation);
  const MomentsSet* ms = nullptr;
  if (sets) for (const MomentsSet& s : sets->moments) if (s.aggregation == aggregation) ms = &s;
  if (!ms) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation %d is not a PG_AGG_VARIANCE", aggregation);
  const bool grouped = result->group_aggregations != nullptr;
  if (grouped ? (group_row < 0 || group_row >= result->num_groups || group_row >= ms->rows) : group_row != -1)
    return fail(PG_ERR_INVALID_ARGUMENT, "group row %d out of range", group_row);
  const pg_agg_value& v = grouped ? result->group_aggregations[(size_t)group_row * (size_t)result->num_aggregations + (size_t)aggregation] : result->aggregations[aggregation];
  *out_count = v.count; *out_sum = v.sum; *out_m2 = ms->m2[(size_t)(grouped ? group_row : 0)];
  return PG_OK;
}

pg_status pg_result_percentile_counts(const pg_result* result, int32_t aggregation, int32_t group_row, const int32_t** out_dict_ids, const uint32_t** out_counts, int32_t* out_num) {
  if (!result || !out_dict_ids || !out_counts || !out_num) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  *out_dict_ids = nullptr; *out_counts = nullptr; *out_num = 0;
  const ResultInternal* lists = static_cast<const ResultInternal*>(result->internal);
  if (aggregation < 0 || aggregation >= result->num_aggregations) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation %d out of range", aggregation);
  const CountList* cl = nullptr;
  if (lists) for (const CountList& l : lists->counts) if (l.aggregation == aggregation) cl = &l;
  if (!cl) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation %d is not a PG_AGG_PERCENTILE", aggregation);
  const bool grouped = result->group_aggregations != nullptr;
  if (grouped ? (group_row < 0 || group_row >= result->num_groups || group_row >= cl->rows) : group_row != -1)
    return fail(PG_ERR_INVALID_ARGUMENT, "group row %d out of range", group_row);
  const size_t row = grouped ? (size_t)group_row : 0, first = cl->offsets[row];
  *out_dict_ids = cl->dict_ids.data() + first;
  *out_counts = cl->counts.data() + first;
  *out_num = (int32_t)(cl->offsets[row + 1] - first);
  return PG_OK;
}

pg_status pg_result_value_counts(const pg_result* result, int32_t aggregation, int32_t group_row, const int64_t** out_value_bits, const uint32_t** out_counts, int32_t* out_num) {
  if (!result || !out_value_bits || !out_counts || !out_num) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  *out_value_bits = nullptr; *out_counts = nullptr; *out_num = 0;
  const ResultInternal* lists = static_cast<const ResultInternal*>(result->internal);
  if (aggregation < 0 || aggregation >= result->num_aggregations) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation %d out of range", aggregation);
  const ValueList* vl = nullptr;
  if (lists) for (const ValueList& l : lists->values) if (l.aggregation == aggregation) vl = &l;
  if (!vl) return fail(PG_ERR_INVALID_ARGUMENT, "aggregation %d is not a PG_AGG_PERCENTILE / PG_AGG_DISTINCTCOUNT on a raw column", aggregation);
  const bool grouped = result->group_aggregations != nullptr;
  if (grouped ? (group_row < 0 || group_row >= result->num_groups || group_row >= vl->rows) : group_row != -1)
    return fail(PG_ERR_INVALID_ARGUMENT, "group row %d out of range", group_row);
  const size_t row = grouped ? (size_t)group_row : 0, first = vl->offsets[row];
  *out_value_bits = vl->value_bits.data() + first;
  *out_counts = vl->counts.data() + first;
  *out_num = (int32_t)(vl->offsets[row + 1] - first);
  return PG_OK;
}

static pg_status check_ordinary_query(const pg_segment* segment, const pg_query* query) {
  if (!(query->flags & PG_QUERY_NULL_HANDLING)) return check_query_plan(segment, query, 0);
  // enableNullHandling: the query that runs is the rewritten one (execute_null_handling): the filter's getTrues() over three-valued
  // leaves, one more IS NOT NULL leaf for every aggregated column that has null docs
  NullRewriter rw{segment};
  FilterExpr root;
  bool has_filter = false;
  pg_status st = parse_filter(query, &root, &has_filter);
  if (st != PG_OK) return st;
  FlatQuery base;
  if (has_filter) base.emit(rw.trues(root));
  base.finish(*query);
  const int na = query->num_aggregations, ng = query->num_group_by;
  if (na < 0 || ng < 0 || (na > 0 && !query->aggregations) || (ng > 0 && !query->group_by_columns)) return fail(PG_ERR_INVALID_ARGUMENT, "bad aggregation / group-by lists");
  bool lanes = false;
  for (int a = 0; a < na; ++a) lanes |= rw.has_nulls(query->aggregations[a].column);
  std::vector<int32_t> keys;
  if (ng > 0) {
    // nullable keys are read through their null-key images (one more digit value each: the key space grows)
    for (int g = 0; g < ng; ++g) {
      const int c = query->group_by_columns[g];
      if (rw.has_nulls(c) && segment->cols[(size_t)c].nullkey_column < 0) return fail(PG_ERR_UNSUPPORTED, "GROUP BY over nullable raw column keeps the CPU plan");
      keys.push_back(rw.has_nulls(c) ? segment->cols[(size_t)c].nullkey_column : c);
    }
    base.q.group_by_columns = keys.data();
  }
  return check_query_plan(segment, &base.q, lanes ? 1 : 0);
}

pg_status pg_filter_bitmap(pg_segment* segment, const pg_query* query, uint64_t* out_words, int64_t num_words, int64_t* out_cardinality) {
  if (!out_words) return fail(PG_ERR_INVALID_ARGUMENT, "null bitmap buffer");
  if (reserved_flags(query)) return fail_reserved_flags(query);
  if (query && (query->flags & PG_QUERY_NULL_HANDLING)) return execute_null_handling(segment, query, nullptr, out_words, num_words, out_cardinality);
  return execute_impl(segment, query, nullptr, nullptr, out_words, num_words, out_cardinality);
}

static pg_status gather_impl(pg_segment* seg, int32_t column, const int32_t* doc_ids, int32_t length, int32_t* out_dict, int32_t* out_int, double* out_double,
                             int64_t* out_long = nullptr) {
  if (!g_engine.initialized) return fail(PG_ERR_NOT_INITIALIZED, "pg_init has not been called");
  if (!seg || (length > 0 && !doc_ids)) return fail(PG_ERR_INVALID_ARGUMENT, "null argument");
  if (column < 0 || column >= (int)seg->cols.size()) return fail(PG_ERR_INVALID_ARGUMENT, "column %d out of range", column);
  if (length <= 0) return PG_OK;
  for (int32_t i = 0; i < length; ++i) if (doc_ids[i] < 0 || doc_ids[i] >= seg->num_docs) return fail(PG_ERR_INVALID_ARGUMENT, "docId %d out of range", doc_ids[i]);
  const ColumnDev& col = seg->cols[(size_t)column];
  if (out_dict && col.encoding != PG_FWD_FIXED_BIT_DICT) return fail(PG_ERR_INVALID_ARGUMENT, "column %s is not dictionary encoded", col.name.c_str());
  if (out_int && col.stored_type != PG_TYPE_INT) return fail(PG_ERR_INVALID_ARGUMENT, "column %s is not INT: use pg_read_long_values / pg_read_double_values", col.name.c_str());
  HIP_TRY(hipSetDevice(phys_device(seg->device)));
  ExecCtx* ctx = nullptr;
  pg_status st = acquire_ctx(seg, &ctx);
  if (st != PG_OK) return st;
  CtxGuard guard{seg, ctx};
  if (ctx->gather_capacity < (size_t)length) {
    if (ctx->d_gather_in) (void)hipFree(ctx->d_gather_in);
    if (ctx->d_gather_out) (void)hipFree(ctx->d_gather_out);
    ctx->d_gather_in = nullptr; ctx->d_gather_out = nullptr; ctx->gather_capacity = 0;
    size_t cap = std::max<size_t>((size_t)length, 16384);
    HIP_TRY(hipMalloc((void**)&ctx->d_gather_in, cap * 4));
    HIP_TRY(hipMalloc((void**)&ctx->d_gather_out, cap * 8));
    ctx->gather_capacity = cap;
  }
  HIP_TRY(hipMemcpyAsync(ctx->d_gather_in, doc_ids, (size_t)length * 4, hipMemcpyHostToDevice, ctx->stream));
  DevColumn dc;
  memset(&dc, 0, sizeof(dc));
  dc.fwd = col.d_fwd; dc.bits = col.bits; dc.is_raw = col.encoding == PG_FWD_RAW_FIXED_BYTE;
  dc.vkind = col.vkind;
  dc.dict = col.vkind == kValI32 ? col.d_dict : reinterpret_cast<const int32_t*>(col.d_dict64);
  dc.cardinality = col.cardinality; dc.dict_bytes = col.cardinality * (col.vkind == kValI32 ? 4 : 8);
  const unsigned blocks = (unsigned)((length + 255) / 256);
  gather_values_kernel<<<dim3(blocks), dim3(256), 0, ctx->stream>>>(dc, (long long)col.value_base, ctx->d_gather_in, length,
      out_dict ? (int32_t*)ctx->d_gather_out : nullptr, out_int ? (int32_t*)ctx->d_gather_out : nullptr,
      out_long ? (long long*)ctx->d_gather_out : nullptr, out_double ? (double*)ctx->d_gather_out : nullptr);
  HIP_TRY(hipGetLastError());
  void* host_out = out_dict ? (void*)out_dict : (out_int ? (void*)out_int : (out_long ? (void*)out_long : (void*)out_double));
  HIP_TRY(hipMemcpyAsync(host_out, ctx->d_gather_out, (size_t)length * ((out_double || out_long) ? 8 : 4), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return PG_OK;
}

pg_status pg_read_dict_ids(pg_segment* segment, int32_t column, const int32_t* doc_ids, int32_t length, int32_t* out_dict_ids) {
  if (!out_dict_ids && length > 0) return fail(PG_ERR_INVALID_ARGUMENT, "null output");
  return gather_impl(segment, column, doc_ids, length, out_dict_ids, nullptr, nullptr);
}
pg_status pg_read_int_values(pg_segment* segment, int32_t column, const int32_t* doc_ids, int32_t length, int32_t* out_values) {
  if (!out_values && length > 0) return fail(PG_ERR_INVALID_ARGUMENT, "null output");
  return gather_impl(segment, column, doc_ids, length, nullptr, out_values, nullptr);
}
pg_status pg_read_long_values(pg_segment* segment, int32_t column, const int32_t* doc_ids, int32_t length, int64_t* out_values) {
  if (!out_values && length > 0) return fail(PG_ERR_INVALID_ARGUMENT, "null output");
  return gather_impl(segment, column, doc_ids, length, nullptr, nullptr, nullptr, out_values);
}
pg_status pg_read_double_values(pg_segment* segment, int32_t column, const int32_t* doc_ids, int32_t length, double* out_values) {
  if (!out_values && length > 0) return fail(PG_ERR_INVALID_ARGUMENT, "null output");
  return gather_impl(segment, column, doc_ids, length, nullptr, nullptr, out_values);
}

}  // extern "C"
