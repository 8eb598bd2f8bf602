// pg_set_pass_layout.h -- the sizes of the set passes' device scratch: the dictId bitsets of DISTINCTCOUNT, the dictId
// counters of PERCENTILE and the HyperLogLog registers of DISTINCTCOUNTHLL.  Plain host C++, no HIP types.
//
// One source for two readers that must agree: the planners (plan_distinct / plan_percentile) price a query's scratch against
// PG_DISTINCT_GROUP_MAX_BYTES / PG_PERCENTILE_GROUP_MAX_BYTES / PG_HLL_GROUP_MAX_BYTES and the group-table budget with these functions, and the
// pass's arm stage (arm_bitsets / arm_hll_raw in pg_engine.hip) allocates with the same ones.  Everything counts 32-bit words; a byte figure is
// the word figure times 4.  (The collect pass's lists are sized by the segment's docs: plan_collect_bytes is a policy bound, not a layout.)
#pragma once
#include <stdint.h>
#include <stddef.h>

namespace pg {

// Words behind the last bitset row: the dictIds a column's WIDTH admits beyond its cardinality (a forward index that breaks the dictionary's
// bound then still writes inside the allocation).
inline size_t distinct_slack_words(int bits, int cardinality) {
  const size_t by_width = (((size_t)1 << bits) + 31) / 32, by_card = ((size_t)(cardinality > 0 ? cardinality : 0) + 31) / 32;
  return (by_width > by_card ? by_width - by_card : 0) + 1;
}
// The same for the 32-bit counters of PERCENTILE (pg_scan_counts.h): 2^bits - cardinality counters behind the last one.
inline size_t counts_slack_words(int bits, int cardinality) {
  const size_t by_width = (size_t)1 << bits, by_card = (size_t)(cardinality > 0 ? cardinality : 0);
  return (by_width > by_card ? by_width - by_card : 0) + 1;
}
// One row of a column: a bit per dictId (DISTINCTCOUNT), or a 32-bit counter per dictId (PERCENTILE).
inline int set_row_words(bool counters, int cardinality) { return counters ? (cardinality > 0 ? cardinality : 0) : (cardinality + 31) / 32; }
inline size_t set_slack_words(bool counters, int bits, int cardinality) { return counters ? counts_slack_words(bits, cardinality) : distinct_slack_words(bits, cardinality); }

// The bitset / counter matrices of a pass, one behind the other: `rows` rows (the raw group ids; 1 without GROUP BY) per column, and behind the
// last row of the last column the largest slack any column asks for.
struct SetMatrixLayout {
  uint64_t row_words = 0, slack_words = 0;
  // one more column; returns its first word
  uint64_t add(bool counters, uint64_t rows, int bits, int cardinality) {
    const uint64_t first = row_words, slack = set_slack_words(counters, bits, cardinality);
    row_words += rows * (uint64_t)set_row_words(counters, cardinality);
    if (slack > slack_words) slack_words = slack;
    return first;
  }
  uint64_t total_words() const { return row_words + slack_words; }
};

// DISTINCTCOUNTHLL.  A register matrix is staged as one 32-bit word per register (the kernels' atomic max), `rows` rows of 2^log2m; behind all
// staged words lie the same registers packed to one byte each -- the only part that is copied to the host.  Behind bitsets (the dictionary
// form: hll_fold_kernel's target) the staged words start sixteen-byte aligned, because hll_pack_kernel reads four registers per load.
inline uint64_t hll_staged_words(uint64_t rows, int log2m) { return rows << log2m; }
inline uint64_t hll_staged_base(uint64_t words_in_front) { return (words_in_front + 3) & ~(uint64_t)3; }
inline uint64_t hll_packed_words(uint64_t staged_words) { return staged_words / 4; }
inline uint64_t hll_scratch_words(uint64_t staged_base, uint64_t staged_words) { return staged_base + staged_words + hll_packed_words(staged_words); }

}  // namespace pg
