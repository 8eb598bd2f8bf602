// Stand-alone check of the set passes' scratch arithmetic (pg_set_pass_layout.h), for a sanitizer build on the CPU (make -C pinot_amd/csrc
// sanitize-layout): the smallest shapes at which the slack, the row widths, the matrix totals and the register areas have an edge.
// Exit status 0 and "ok" when every expectation holds.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../pg_set_pass_layout.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using namespace pg;

int main() {
  // cardinality 0, 1, 31, 32, 33 at the width that just holds its dictIds and at one bit more: {bits, cardinality, bitset row, bitset slack, counter slack}
  const struct { int bits, cardinality; int row_words; size_t distinct_slack, counts_slack; } edges[] = {
      {1, 0, 0, 2, 3},  {2, 0, 0, 2, 5},      // an empty dictionary: every dictId the width admits is beyond the bound
      {1, 1, 1, 1, 2},  {2, 1, 1, 1, 4},
      {5, 31, 1, 1, 2}, {6, 31, 1, 2, 34},    // one word of bits; six bits reach a second word
      {5, 32, 1, 1, 1}, {6, 32, 1, 2, 33},    // the width's dictIds exactly: only the + 1 is left
      {6, 33, 2, 1, 32}, {7, 33, 2, 3, 96},   // a second word of bits
  };
  for (const auto& e : edges) {
    EXPECT(distinct_slack_words(e.bits, e.cardinality) == e.distinct_slack);
    EXPECT(counts_slack_words(e.bits, e.cardinality) == e.counts_slack);
    EXPECT(set_row_words(false, e.cardinality) == e.row_words);
    EXPECT(set_row_words(true, e.cardinality) == e.cardinality);
    EXPECT(set_slack_words(false, e.bits, e.cardinality) == e.distinct_slack && set_slack_words(true, e.bits, e.cardinality) == e.counts_slack);
    // one column, one row: the row and its slack
    SetMatrixLayout one;
    EXPECT(one.add(false, 1, e.bits, e.cardinality) == 0 && one.total_words() == (uint64_t)e.row_words + e.distinct_slack);
  }
  EXPECT(distinct_slack_words(6, 33) == 1 && counts_slack_words(6, 33) == 32 && distinct_slack_words(7, 33) == 3);
  // rows 1 and 3, two columns (33 dictIds in 6 bits, 31 in 5): the columns' first words are the running sums, the total is
  // sum(rows x row words) + the largest slack
  for (const uint64_t rows : {(uint64_t)1, (uint64_t)3}) {
    SetMatrixLayout bits;
    EXPECT(bits.add(false, rows, 6, 33) == 0);
    EXPECT(bits.add(false, rows, 5, 31) == rows * 2);
    EXPECT(bits.row_words == rows * 3 && bits.slack_words == 1 && bits.total_words() == rows * 3 + 1);
    SetMatrixLayout counters;
    EXPECT(counters.add(true, rows, 6, 33) == 0);
    EXPECT(counters.add(true, rows, 5, 31) == rows * 33);
    EXPECT(counters.row_words == rows * 64 && counters.slack_words == 32 && counters.total_words() == rows * 64 + 32);
    // (the larger slack wins whichever column brings it)
    SetMatrixLayout swapped;
    EXPECT(swapped.add(true, rows, 5, 31) == 0 && swapped.add(true, rows, 6, 33) == rows * 31 && swapped.total_words() == counters.total_words());
  }
  {
    SetMatrixLayout bits;
    bits.add(false, 3, 6, 33); bits.add(false, 3, 5, 31);
    EXPECT(bits.total_words() == 10);
    // an HLL fold behind these bitsets: the staged words start at the total rounded up to four words; packed bytes behind them
    const uint64_t base = hll_staged_base(bits.total_words()), staged = hll_staged_words(3, 4);
    EXPECT(base == 12 && staged == 48 && hll_packed_words(staged) == 12 && hll_scratch_words(base, staged) == 12 + 48 + 12);
    // two folds: their matrices follow one another
    EXPECT(hll_scratch_words(base, staged + hll_staged_words(3, 5)) == 12 + 144 + 36);
  }
  EXPECT(hll_staged_base(0) == 0 && hll_staged_base(1) == 4 && hll_staged_base(3) == 4 && hll_staged_base(4) == 4 && hll_staged_base(5) == 8);
  // the raw HLL form: nothing in front of the registers
  EXPECT(hll_staged_words(1, 4) == 16 && hll_scratch_words(0, hll_staged_words(1, 4)) == 20);
  EXPECT(hll_staged_words(2, 4) == 32 && hll_scratch_words(0, hll_staged_words(2, 4)) == 40);
  EXPECT(hll_staged_words(1, 12) == 4096 && hll_scratch_words(0, hll_staged_words(1, 12)) == 5120);
  EXPECT(hll_staged_words(2, 12) == 8192 && hll_scratch_words(0, hll_staged_words(2, 12)) == 10240);
  // two slots (log2m 4 and 12) over two rows
  EXPECT(hll_scratch_words(0, hll_staged_words(2, 4) + hll_staged_words(2, 12)) == 8224 + 2056);
  if (failures == 0) printf("ok\n");
  return failures == 0 ? 0 : 1;
}
