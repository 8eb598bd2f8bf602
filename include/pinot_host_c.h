/* pinot_host_c.h -- C entry points of libpinot_host.so, the C++ mirror of the reference's HOST side of this path
 * (pinot_amd/csrc/host/pinot_host.h: dictionaries, predicate evaluators, QueryContext, GpuPlanMaker, operators, results blocks,
 * combine, the v1 / v3 segment-directory loader) plus the writers that produce columns in Pinot's on-disk layouts.
 *
 * This is NOT the drop-in boundary -- that is include/pinot_gpu.h, which a JNI shim binds.  These functions exist so
 * that the mirror can be driven from tests and tools without a JVM: SQL text in, JSON results out.  Status codes: 0 ok,
 * 1 QueryException (bad query / bad segment), 2 UnsupportedOperationException (plan-time fallback to the CPU plan), 3 other.
 * Strings returned as char* are malloc'ed: release them with ph_free.  ph_last_error() is per thread. */
#ifndef PINOT_HOST_C_H
#define PINOT_HOST_C_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* ph_last_error(void);
void ph_free(char* p);

/* ---- ImmutableSegment built from caller-owned buffers (IndexSegment / DataSource, pinot-segment-spi) ---- */
void* ph_segment_create(const char* name, int32_t num_docs);
int32_t ph_segment_add_int_column(void* seg, const char* name, int32_t has_dictionary, int32_t bits, int32_t cardinality, const void* fwd,
                                  uint64_t fwd_size, const void* dict, uint64_t dict_size, const void* inv, uint64_t inv_size);
/* data_type: pg_data_type (INT, LONG, FLOAT, DOUBLE); dictionary columns pass the big-endian fixed-width .dict buffer */
int32_t ph_segment_add_numeric_column(void* seg, const char* name, int32_t data_type, int32_t has_dictionary, int32_t bits, int32_t cardinality,
                                      const void* fwd, uint64_t fwd_size, const void* dict, uint64_t dict_size, const void* inv, uint64_t inv_size);
/* values: the dictionary's strings in dictId order, each NUL-terminated */
int32_t ph_segment_add_string_column(void* seg, const char* name, int32_t bits, int32_t cardinality, const void* fwd, uint64_t fwd_size,
                                     const char* values, const void* inv, uint64_t inv_size);
/* the <column>.bitmap.nullvalue file of a column added before (DataSource.getNullValueVector) */
int32_t ph_segment_set_null_vector(void* seg, const char* column, const void* data, uint64_t size);
int32_t ph_segment_load(void* seg, int32_t device);                 /* pg_segment_open; device -1: stay on the host (CPU tests) */
void ph_segment_destroy(void* seg);                                 /* IndexSegment.destroy() */

/* ---- ImmutableSegmentLoader.load(indexDir): v1 file-per-index or v3 columns.psf + index_map ---- */
void* ph_segment_load_directory(const char* index_dir, int32_t device, int32_t* status);
char* ph_segment_describe(void* segment, int32_t* status);          /* JSON: columns, types, indexes, what was not offloaded */

/* ---- GpuPlanMaker (InstancePlanMakerImplV2.makeSegmentPlanNode) + combine ---- */
int32_t ph_plan_maker_init(int32_t device, int32_t time_kernels);
/* gpu.devices ("0-7", "0,2,4", "0-3,6") parsed, and the device each of `count` segments of the given sizes goes to when opened in that
 * order (least resident bytes first; an entry -(device << 48 | bytes) gives bytes back): JSON {"devices": [...], "placement": [...]}.
 * No device is touched. */
char* ph_plan_maker_placement(const char* devices_text, const int64_t* segment_bytes, int32_t count, int32_t* status);
char* ph_parse_sql(const char* sql, int32_t* status);               /* QueryContextConverterUtils.getQueryContext for the SQL subset */
char* ph_lower_predicate(const char* sql_predicate, const void* dict, int32_t cardinality, int32_t* status);   /* PredicateEvaluatorProvider */
/* the physical filter operator tree of the WHERE clause (FilterPlanNode + FilterOperatorUtils: leaf operator per predicate, MatchAll / Empty folding,
 * AND children by priority) as text; the segment need not be loaded on a device */
char* ph_explain_filter(void* segment, const char* sql, int32_t* status);
/* The queryable (valid) docIds of an upsert / dedup table's segment -- SegmentContext.getQueryableDocIdsSnapshot(), one serialized
 * RoaringBitmap, copied; NULL clears the set.  From then on every filter over the segment is FilterPlanNode.run()'s (:88-106)
 * AND(user filter, BITMAP(queryableDocIds)), the leaf alone for a query without a filter: ph_explain_filter shows it, ph_execute_sql runs it
 * (on a loaded segment the bitmap is a doc set of the device copy, include/pinot_gpu.h pg_doc_set_create; a segment that is not loaded on
 * a device is declined as before: the mirror has no CPU evaluation path).  A docId >= numDocs is refused when the bitmap reaches the device. */
int32_t ph_segment_set_queryable_doc_ids(void* segment, const void* roaring_bytes, uint64_t size);
/* RangePredicateEvaluatorFactory.newDictionaryBasedEvaluator over an INT dictionary; bounds as strings, "*" = unbounded */
char* ph_lower_range_predicate(const void* dict, int32_t cardinality, const char* lower, int32_t lower_inclusive, const char* upper, int32_t upper_inclusive, int32_t* status);
/* the raw-value range evaluator of an INT (0) / LONG (1) column: inclusive [rawLower, rawUpper] */
char* ph_lower_raw_range_predicate(int32_t data_type, const char* lower, int32_t lower_inclusive, const char* upper, int32_t upper_inclusive, int32_t* status);
/* the LDS membership table of a PG_PRED_RAW_SET leaf, built from `members` (distinct 4- / 8-byte bit patterns) and probed as the kernels probe it:
 * out_hits[i] = probes[i] found; returns the bucket count (0: no table) */
int32_t ph_raw_set_table_probe(int32_t key_bytes, const uint64_t* members, int32_t num_members, const uint64_t* probes, int64_t num_probes, uint8_t* out_hits);
char* ph_execute_sql(void** segments, int32_t num_segments, const char* sql, int32_t max_execution_threads, int32_t* status);

/* ---- DataTable V4 (DataTableImplV4.toBytes of the intermediate results: what the server sends the broker; host/datatable_v4.cpp) ---- */
/* malloc-ed buffer of *out_size bytes (ph_free), or NULL with *status set */
uint8_t* ph_execute_sql_datatable(void** segments, int32_t num_segments, const char* sql, int32_t max_execution_threads, int64_t* out_size, int32_t* status);
/* the writer alone, over a results block given as flat arrays (CPU tests): see host/c_api.cpp for the array layouts */
uint8_t* ph_datatable_v4_build(int32_t is_group_by, int32_t num_functions, const int32_t* function_types, const char* const* function_columns, int32_t num_keys,
                               const char* const* key_names, const int32_t* key_types, int64_t num_rows, const int64_t* key_longs, const double* key_doubles,
                               const char* const* key_strings, const int64_t* counts, const double* sums, const double* mins, const double* maxs,
                               const uint8_t* is_null, const int64_t* stats, int32_t null_handling, int32_t limit_reached, int32_t segments_processed,
                               int32_t segments_matched, int64_t* out_size, int32_t* status);

/* ---- the group-by table behind the combine operator and the broker's reducer (IndexedTable / TableResizer / GroupByUtils; host/indexed_table.cpp) ---- */
/* GroupByCombineOperator + GroupByDataTableReducer over group-by blocks given as flat arrays (block b = the next block_rows[b] rows); `sql` supplies
 * aggregations, GROUP BY, ORDER BY, LIMIT and the trim options.  JSON: {"combined": block, "reduced": rows, "table": sizes}; ph_free it. */
char* ph_group_by_combine(const char* sql, int32_t num_blocks, const int64_t* block_rows, const int32_t* key_types, const int64_t* key_longs,
                          const double* key_doubles, const char* const* key_strings, const uint8_t* key_is_null, const int64_t* counts, const double* sums,
                          const double* mins, const double* maxs, const uint8_t* is_null, int32_t* status);
/* The same with the cells of DISTINCTCOUNT functions given as value sets: cell (row, function) holds the LONG values
 * set_values[set_offsets[row * functions + function] .. set_offsets[.. + 1]); the combine merges them by union, the final result is the size. */
char* ph_group_by_combine_sets(const char* sql, int32_t num_blocks, const int64_t* block_rows, const int32_t* key_types, const int64_t* key_longs,
                          const double* key_doubles, const char* const* key_strings, const uint8_t* key_is_null, const int64_t* counts, const double* sums,
                          const double* mins, const double* maxs, const uint8_t* is_null, const int64_t* set_offsets, const int64_t* set_values, int32_t* status);
/* The combine of PERCENTILE value lists: cell (row, function) of a PERCENTILE function holds the runs (run_values[i], run_counts[i]) for i in
 * [run_offsets[row * functions + function], run_offsets[.. + 1]); the combine merges them run-wise, the final result is the percentile of `sql`.
 * GROUP BY: as ph_group_by_combine; aggregation only: one row per block, {"combined": <block>}. */
char* ph_combine_counts(const char* sql, int32_t num_blocks, const int64_t* block_rows, const int32_t* key_types, const int64_t* key_longs,
                        const double* key_doubles, const char* const* key_strings, const uint8_t* key_is_null, const int64_t* counts, const double* sums,
                        const double* mins, const double* maxs, const uint8_t* is_null, const int64_t* run_offsets, const double* run_values,
                        const int64_t* run_counts, int32_t* status);
/* The combine of DISTINCTCOUNTHLL sketches: cell (row, function) of a DISTINCTCOUNTHLL function holds the registers registers[register_offsets[row *
 * functions + function] .. register_offsets[.. + 1]) -- 2^log2m bytes, one rank each (pg_result_hll_registers' format), or none for an empty sketch;
 * the combine merges them by the register-wise max, the final result is the estimate (a LONG).  GROUP BY: as ph_group_by_combine; aggregation
 * only: one row per block, {"combined": <block>}. */
char* ph_combine_hll(const char* sql, int32_t num_blocks, const int64_t* block_rows, const int32_t* key_types, const int64_t* key_longs,
                     const double* key_doubles, const char* const* key_strings, const uint8_t* key_is_null, const int64_t* counts, const double* sums,
                     const double* mins, const double* maxs, const uint8_t* is_null, const int64_t* register_offsets, const uint8_t* registers, int32_t* status);
/* The combine of VarianceTuples (VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP): cell (row, function) of such a function holds the tuple (counts[at],
 * sums[at], m2s[at]); the combine merges tuples with VarianceTuple.apply(VarianceTuple), the final result is m2 / n, m2 / (n - 1) or their square
 * root (-Infinity for no doc, and for one doc in the sample forms).  GROUP BY: as ph_group_by_combine; aggregation only: one row per block,
 * {"combined": <block>}. */
char* ph_combine_moments(const char* sql, int32_t num_blocks, const int64_t* block_rows, const int32_t* key_types, const int64_t* key_longs,
                         const double* key_doubles, const char* const* key_strings, const uint8_t* key_is_null, const int64_t* counts, const double* sums,
                         const double* mins, const double* maxs, const uint8_t* is_null, const double* m2s, int32_t* status);
/* HyperLogLog.cardinality() of num_registers = 2^log2m registers; -1 when num_registers is not such a count. */
int64_t ph_hll_cardinality(const uint8_t* registers, int32_t num_registers);
/* The registers (2^log2m bytes) after offering `num` longs to an empty sketch, computed with the header the kernels include; 0, or 1 for a bad log2m. */
int32_t ph_hll_offer_longs(const int64_t* longs, int64_t num, int32_t log2m, uint8_t* out_registers);
/* The 32 stored bits of a FLOAT dictionary entry from the bits of the double it was widened to (a NaN keeps its payload). */
uint32_t ph_hll_float_bits_of_widened(uint64_t double_bits);
/* The sorted runs of a raw column (pg_result_value_counts: value bits, counts) as the intermediate results that segments merge, without a device.
 * stored_type: 0 INT, 1 LONG, 2 FLOAT, 3 DOUBLE.  PERCENTILE's list: runs of (double, count) as getDoubleValuesSV gives the values -- two LONGs on one
 * double merge into one run; DISTINCTCOUNT's set: the stored type's 64-bit images, ascending as longs.  The out arrays hold `num` entries; returns
 * how many were written. */
int32_t ph_value_counts_from_device(int32_t stored_type, const int64_t* value_bits, const uint32_t* counts, int32_t num, double* out_values, int64_t* out_counts);
int32_t ph_value_set_from_device(int32_t stored_type, const int64_t* value_bits, int32_t num, int64_t* out_values);
int32_t ph_group_by_table_capacity(int32_t limit, int32_t min_num_groups);          /* GroupByUtils.getTableCapacity */
int32_t ph_group_by_trim_threshold(int32_t trim_size, int32_t trim_threshold);      /* GroupByUtils.getIndexedTableTrimThreshold */

/* ---- writers in the reference's layouts (FixedBitSVForwardIndexWriter, SegmentDictionaryCreator, FixedByteChunkForwardIndexWriter v2,
 *      BitmapInvertedIndexWriter, RoaringBitmap portable serialization) and the synthetic-column generator of the benchmarks ---- */
int32_t ph_num_bits_per_value(int32_t max_value);
int64_t ph_fixedbit_size(int64_t num_docs, int32_t bits);
void ph_fixedbit_pack(const int32_t* dict_ids, int64_t num_docs, int32_t bits, uint8_t* out, int32_t threads);
void ph_generate_packed_uniform(uint64_t seed, int64_t num_docs, int32_t cardinality, int32_t bits, uint8_t* out, int32_t threads);
void ph_generate_uniform(uint64_t seed, int64_t start, int64_t count, int32_t cardinality, int32_t* out);
void ph_dict_write_int(const int32_t* sorted_values, int32_t length, uint8_t* out);
void ph_dict_write_fixed(const void* sorted_values, int32_t length, int32_t entry_size, uint8_t* out);
int64_t ph_raw_size_v2(int32_t num_docs, int32_t num_docs_per_chunk);
void ph_raw_write_int_v2(const int32_t* values, int32_t num_docs, int32_t num_docs_per_chunk, uint8_t* out);
int64_t ph_raw_size_fixed_v2(int32_t num_docs, int32_t num_docs_per_chunk, int32_t entry_size);
void ph_raw_write_fixed_v2(const void* values, int32_t num_docs, int32_t num_docs_per_chunk, int32_t entry_size, uint8_t* out);
int64_t ph_roaring_serialize(const int32_t* sorted_doc_ids, int64_t n, int32_t run_optimize, uint8_t* out);     /* out NULL: size only */
int64_t ph_inverted_build(const int32_t* dict_ids, int32_t num_docs, int32_t cardinality, int32_t run_optimize, uint8_t* out);

/* ---- chunk-compressed raw forward indexes (pinot_amd/csrc/pg_chunk_codec.h: the parsers the device kernel shares, and the host decoder) ----
 * codec: ChunkCompressionType value, 1 SNAPPY | 3 LZ4.  ph_chunk_decode: one chunk into exactly `expect` bytes; 1 when it decoded to exactly
 * that size, otherwise the parser's error code (2..10).  ph_raw_decode_file: a whole version 1..4 file of num_docs docs into its
 * num_docs * sizeOfEntry big-endian value bytes; 0 ok, 1 header / offset table rejected, 2 codec not decoded, 3 malformed chunk. */
int32_t ph_chunk_decode(int32_t codec, const uint8_t* src, uint32_t size, uint8_t* dst, uint32_t expect);
int32_t ph_raw_decode_file(const uint8_t* file, uint64_t size, int64_t num_docs, uint8_t* out_values);

#ifdef __cplusplus
}
#endif
#endif
