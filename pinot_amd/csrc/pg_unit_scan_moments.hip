// Instantiates scan_moments_kernel and group_moments_kernel: VARIANCE's pivoted moments -- see pg_launch.h.
#include "pg_scan_moments.h"
#include "pg_launch.h"

namespace pg {

static_assert(sizeof(MomentsParams) <= 4096, "the parameter block is a kernel argument");

void launch_scan_moments(int blocks, size_t lds, hipStream_t stream, const MomentsParams& mp) {
  scan_moments_kernel<<<dim3((unsigned)blocks), dim3(kMomentsBlockThreads), lds, stream>>>(mp);
}

int waves_scan_moments() {
  static const int cap = max_waves_per_cu(scan_moments_kernel);
  return cap;
}

void launch_group_moments(int blocks, size_t lds, hipStream_t stream, const MomentsParams& mp) {
  group_moments_kernel<<<dim3((unsigned)blocks), dim3(kMomentsBlockThreads), lds, stream>>>(mp);
}

int waves_group_moments() {
  static const int cap = max_waves_per_cu(group_moments_kernel);
  return cap;
}

}  // namespace pg
