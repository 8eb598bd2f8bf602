// Instantiates scan_simple_valid_kernel -- see pg_launch.h.  A unit of its own: scan_simple_kernel and scan_simple_set_kernel keep
// their code and registers (pg_scan_simple.h).
#include "pg_scan_simple.h"
#include "pg_launch.h"

namespace pg {

// scan_simple_kernel's shape behind one PG_PRED_DOC_SET leaf: `range leaf AND doc set` (or the doc set alone) in front of at most one
// aggregated packed column.
__global__ __launch_bounds__(kWideBlockThreads, PG_SIMPLE_WAVES) void scan_simple_valid_kernel(const ScanParams p) {
  __shared__ BlockPartial red[kWideBlockThreads / 64];
  __shared__ uint32_t fold_flag;
  scan_simple_body<false, true, false>(p, blockIdx.x, gridDim.x, red, &fold_flag);
}

// The same, and a tile without a valid doc skips its filter column too (PINOT_GPU_SCAN_SIMPLE_VALID=2: kept for the measurement).
__global__ __launch_bounds__(kWideBlockThreads, PG_SIMPLE_WAVES) void scan_simple_valid_skip_kernel(const ScanParams p) {
  __shared__ BlockPartial red[kWideBlockThreads / 64];
  __shared__ uint32_t fold_flag;
  scan_simple_body<false, true, true>(p, blockIdx.x, gridDim.x, red, &fold_flag);
}

void launch_scan_simple_valid(int blocks, int threads, hipStream_t stream, const ScanParams& p, bool skip_empty_tiles) {
  if (skip_empty_tiles) scan_simple_valid_skip_kernel<<<dim3((unsigned)blocks), dim3((unsigned)threads), 0, stream>>>(p);
  else scan_simple_valid_kernel<<<dim3((unsigned)blocks), dim3((unsigned)threads), 0, stream>>>(p);
}

int waves_scan_simple_valid() {
  static const int cap = std::min(max_waves_per_cu_lean(scan_simple_valid_kernel), max_waves_per_cu_lean(scan_simple_valid_skip_kernel));
  return cap;
}

}  // namespace pg
