// Instantiates scan_distinct_kernel (both tiers) and group_distinct_kernel: DISTINCTCOUNT as dictId bitsets -- see pg_launch.h.
#include "pg_scan_distinct.h"
#include "pg_launch.h"

namespace pg {

void launch_scan_distinct(bool lds_tier, int blocks, size_t lds, hipStream_t stream, const DistinctParams& dp) {
  if (lds_tier) {
    set_dynamic_lds(scan_distinct_kernel<true>, lds);
    scan_distinct_kernel<true><<<dim3((unsigned)blocks), dim3(kHistBlockThreads), lds, stream>>>(dp);
  } else {
    scan_distinct_kernel<false><<<dim3((unsigned)blocks), dim3(kDistinctBlockThreads), lds, stream>>>(dp);
  }
}

int waves_scan_distinct(bool lds_tier) {
  static const int cap_lds = max_waves_per_cu(scan_distinct_kernel<true>);
  static const int cap_hbm = max_waves_per_cu(scan_distinct_kernel<false>);
  return lds_tier ? cap_lds : cap_hbm;
}

void launch_group_distinct(int blocks, size_t lds, hipStream_t stream, const DistinctParams& dp) {
  group_distinct_kernel<<<dim3((unsigned)blocks), dim3(kDistinctBlockThreads), lds, stream>>>(dp);
}

int waves_group_distinct() {
  static const int cap = max_waves_per_cu(group_distinct_kernel);
  return cap;
}

}  // namespace pg
