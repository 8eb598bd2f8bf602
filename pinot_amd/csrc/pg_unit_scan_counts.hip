// Instantiates scan_counts_kernel (both tiers) and group_counts_kernel: PERCENTILE as dictId count histograms -- see pg_launch.h.
#include "pg_scan_counts.h"
#include "pg_launch.h"

namespace pg {

void launch_scan_counts(bool lds_tier, int blocks, size_t lds, hipStream_t stream, const DistinctParams& dp) {
  if (lds_tier) {
    set_dynamic_lds(scan_counts_kernel<true>, lds);
    scan_counts_kernel<true><<<dim3((unsigned)blocks), dim3(kHistBlockThreads), lds, stream>>>(dp);
  } else {
    scan_counts_kernel<false><<<dim3((unsigned)blocks), dim3(kDistinctBlockThreads), lds, stream>>>(dp);
  }
}

int waves_scan_counts(bool lds_tier) {
  static const int cap_lds = max_waves_per_cu(scan_counts_kernel<true>);
  static const int cap_hbm = max_waves_per_cu(scan_counts_kernel<false>);
  return lds_tier ? cap_lds : cap_hbm;
}

void launch_group_counts(int blocks, size_t lds, hipStream_t stream, const DistinctParams& dp) {
  group_counts_kernel<<<dim3((unsigned)blocks), dim3(kDistinctBlockThreads), lds, stream>>>(dp);
}

int waves_group_counts() {
  static const int cap = max_waves_per_cu(group_counts_kernel);
  return cap;
}

}  // namespace pg
