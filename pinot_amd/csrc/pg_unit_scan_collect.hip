// Instantiates scan_collect_kernel / group_collect_kernel and the sort + run-length encoding behind them: PERCENTILE / DISTINCTCOUNT on raw
// columns as sorted (value, count) runs -- see pg_launch.h.
#include "pg_scan_collect.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "pg_launch.h"

namespace pg {

void launch_scan_collect(int blocks, size_t lds, hipStream_t stream, const CollectParams& cp) {
  scan_collect_kernel<<<dim3((unsigned)blocks), dim3(kDistinctBlockThreads), lds, stream>>>(cp);
}

int waves_scan_collect() {
  static const int cap = max_waves_per_cu(scan_collect_kernel);
  return cap;
}

void launch_group_collect(int blocks, size_t lds, hipStream_t stream, const CollectParams& cp) {
  group_collect_kernel<<<dim3((unsigned)blocks), dim3(kDistinctBlockThreads), lds, stream>>>(cp);
}

int waves_group_collect() {
  static const int cap = max_waves_per_cu(group_collect_kernel);
  return cap;
}

// rocPRIM's scratch for a list of n entries: the largest of the three calls' (sizing calls launch nothing).
hipError_t collect_sort_temp_bytes(size_t n, bool grouped, size_t* out_bytes) {
  size_t need = 0, bytes = 0;
  unsigned long long* k64 = nullptr;
  uint32_t* k32 = nullptr;
  hipError_t e = hipSuccess;
  if (grouped) {
    e = rocprim::radix_sort_pairs(nullptr, bytes, k64, k64, k32, k32, n, 0u, 64u, nullptr);
    if (e != hipSuccess) return e;
    need = std::max(need, bytes);
    e = rocprim::radix_sort_pairs(nullptr, bytes, k32, k32, k64, k64, n, 0u, 32u, nullptr);
    if (e != hipSuccess) return e;
    need = std::max(need, bytes);
  } else {
    e = rocprim::radix_sort_keys(nullptr, bytes, k64, k64, n, 0u, 64u, nullptr);
    if (e != hipSuccess) return e;
    need = std::max(need, bytes);
  }
  e = rocprim::inclusive_scan(nullptr, bytes, k32, k32, n, rocprim::plus<uint32_t>(), nullptr);
  if (e != hipSuccess) return e;
  *out_bytes = std::max(need, bytes);
  return hipSuccess;
}

hipError_t collect_sort_runs(const CollectSort& s, size_t n, int num_cus, hipStream_t stream, CollectRuns* out) {
  if (n == 0) return hipErrorInvalidValue;
  size_t bytes = s.temp_bytes;
  const unsigned long long* sorted = nullptr;
  const uint32_t* sorted_rows = nullptr;
  hipError_t e;
  if (s.rows != nullptr) {
    // stable by image carrying the row, then stable by row over the bits the raw group ids need: ascending (row, image)
    e = rocprim::radix_sort_pairs(s.temp, bytes, s.images, s.images_work, s.rows, s.rows_a, n, 0u, 64u, stream);
    if (e != hipSuccess) return e;
    bytes = s.temp_bytes;
    e = rocprim::radix_sort_pairs(s.temp, bytes, s.rows_a, s.rows_b, s.images_work, s.images, n, 0u, (unsigned)s.row_bits, stream);
    if (e != hipSuccess) return e;
    sorted = s.images; sorted_rows = s.rows_b;
    out->images = s.images_work; out->rows = s.rows_a;      // (both are free again)
  } else {
    e = rocprim::radix_sort_keys(s.temp, bytes, s.images, s.images_work, n, 0u, 64u, stream);
    if (e != hipSuccess) return e;
    sorted = s.images_work;
    out->images = s.images; out->rows = nullptr;
  }
  const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)num_cus * 16));
  collect_run_heads_kernel<<<dim3(grid), dim3(256), 0, stream>>>(sorted, sorted_rows, (unsigned long long)n, s.heads);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  bytes = s.temp_bytes;
  e = rocprim::inclusive_scan(s.temp, bytes, s.heads, s.position, n, rocprim::plus<uint32_t>(), stream);
  if (e != hipSuccess) return e;
  // (the heads are spent: their array takes the runs' first indices)
  collect_run_compact_kernel<<<dim3(grid), dim3(256), 0, stream>>>(sorted, sorted_rows, s.position, (unsigned long long)n, out->images, s.heads, out->rows, s.num_runs);
  out->first = s.heads;
  return hipGetLastError();
}

}  // namespace pg
