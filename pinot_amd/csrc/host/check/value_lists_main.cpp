// Stand-alone check of the host mirror's raw-column intermediate results, for a sanitizer build on the CPU (make -C pinot_amd/csrc sanitize-host):
// ValueCounts::fromDeviceValues / ValueSet::fromDeviceValues over the runs pg_result_value_counts returns, and the combine's merges over them.
// Exit status 0 and "ok" when every expectation holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../../include/pinot_host_c.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static int64_t bits_of(double v) { int64_t b; memcpy(&b, &v, 8); return b; }

int main() {
  // two LONGs on one double: one run of the list, two elements of the set
  const int64_t a = 1ll << 53, b = (1ll << 53) + 1;
  const int64_t long_bits[] = {INT64_MIN, -7, 5, a, b, INT64_MAX};
  const uint32_t long_counts[] = {1, 2, 1, 2, 3, 4};
  double values[6]; int64_t counts[6], set[6];
  int32_t n = ph_value_counts_from_device(1, long_bits, long_counts, 6, values, counts);
  EXPECT(n == 5 && values[3] == (double)a && counts[3] == 5 && counts[4] == 4 && values[0] == (double)INT64_MIN);
  n = ph_value_set_from_device(1, long_bits, 6, set);
  EXPECT(n == 6 && set[3] == a && set[4] == b);
  // FLOAT / DOUBLE in Double.compare's order: -0.0 and 0.0 stay two runs; the set ascends as 64-bit images
  const int64_t dbl_bits[] = {bits_of(-1.0 / 0.0), bits_of(-1.5), bits_of(-0.0), bits_of(0.0), bits_of(2.5), bits_of(1.0 / 0.0), 0x7FF8000000000000ll};
  const uint32_t dbl_counts[] = {1, 1, 2, 3, 1, 1, 9};
  double dv[7]; int64_t dc[7], ds[7];
  n = ph_value_counts_from_device(3, dbl_bits, dbl_counts, 7, dv, dc);
  EXPECT(n == 7 && dc[2] == 2 && dc[3] == 3 && dv[6] != dv[6] && dc[6] == 9);
  n = ph_value_set_from_device(3, dbl_bits, 7, ds);
  EXPECT(n == 7);
  for (int i = 1; i < n; ++i) EXPECT(ds[i - 1] < ds[i]);
  // nothing matched
  EXPECT(ph_value_counts_from_device(0, nullptr, nullptr, 0, values, counts) == 0 && ph_value_set_from_device(2, nullptr, 0, set) == 0);
  // the combine over three segments' raw-derived lists: one PERCENTILE function, one row per block, run-wise merge and the final result
  {
    const int64_t block_rows[] = {1, 1, 1};
    const int64_t cell_counts[] = {3, 0, 9};
    const double zeros[] = {0, 0, 0};
    const uint8_t not_null[] = {0, 0, 0};
    const int64_t run_offsets[] = {0, 2, 2, 5};                       // the second segment matched nothing
    const double run_values[] = {-7.0, 5.0, (double)a, 5.0, 9.0};     // (any order inside a cell)
    const int64_t run_counts[] = {2, 1, 5, 3, 1};
    int32_t status = -1;
    char* json = ph_combine_counts("SELECT PERCENTILE50(m) FROM t", 3, block_rows, nullptr, nullptr, nullptr, nullptr, nullptr, cell_counts, zeros, zeros, zeros, not_null,
                             run_offsets, run_values, run_counts, &status);
    EXPECT(status == 0 && json != nullptr);
    if (json) {
      EXPECT(strstr(json, "\"counts\": [2, 4, 1, 5]") != nullptr);      // -7 x2, 5 x(1 + 3), 9 x1, 2^53 x5
      EXPECT(strstr(json, "\"final\": [9]") != nullptr);                // 12 values, index 6: -7 -7 5 5 5 5 [9]
      ph_free(json);
    }
  }
  // NaN in both segments' lists (a raw DOUBLE column): it sorts last, merges into one run, and the merge ends
  {
    const int64_t block_rows[] = {1, 1};
    const int64_t cell_counts[] = {3, 4};
    const double zeros[] = {0, 0};
    const uint8_t not_null[] = {0, 0};
    const int64_t run_offsets[] = {0, 2, 4};
    const double nan = dv[6];
    const double run_values[] = {1.0, nan, 0.5, nan};
    const int64_t run_counts[] = {1, 2, 1, 3};
    int32_t status = -1;
    char* json = ph_combine_counts("SELECT PERCENTILE100(m) FROM t", 2, block_rows, nullptr, nullptr, nullptr, nullptr, nullptr, cell_counts, zeros, zeros, zeros, not_null,
                                   run_offsets, run_values, run_counts, &status);
    EXPECT(status == 0 && json != nullptr);
    if (json) {
      EXPECT(strstr(json, "\"counts\": [1, 1, 5]") != nullptr && strstr(json, "\"final\": [\"NaN\"]") != nullptr);
      ph_free(json);
    }
  }
  if (failures == 0) printf("ok\n");
  return failures == 0 ? 0 : 1;
}
