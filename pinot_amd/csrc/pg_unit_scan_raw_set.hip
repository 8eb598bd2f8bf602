// Instantiates scan_raw_set_kernel<4 | 8> and raw_set_bitmap_kernel<4 | 8> -- see pg_launch.h.
#include "pg_scan_raw_set.h"
#include "pg_launch.h"

namespace pg {

template <int kKeyBytes>
__global__ __launch_bounds__(kBlockThreads, PG_RAW_SET_WAVES) void scan_raw_set_kernel(const ScanParams p) {
  __shared__ BlockPartial red[kBlockThreads / 64];
  __shared__ uint32_t fold_flag;
  scan_raw_set_body<kKeyBytes>(p, red, &fold_flag);
}

template <int kKeyBytes>
__global__ __launch_bounds__(kBlockThreads, PG_RAW_SET_WAVES) void raw_set_bitmap_kernel(const RawSetBitmapParams p) {
  raw_set_bitmap_body<kKeyBytes>(p);
}

void launch_scan_raw_set(int key_bytes, int blocks, size_t table_bytes, hipStream_t stream, const ScanParams& p) {
  if (key_bytes == 4) {
    set_dynamic_lds(scan_raw_set_kernel<4>, table_bytes);
    scan_raw_set_kernel<4><<<dim3((unsigned)blocks), dim3(kBlockThreads), table_bytes, stream>>>(p);
  } else {
    set_dynamic_lds(scan_raw_set_kernel<8>, table_bytes);
    scan_raw_set_kernel<8><<<dim3((unsigned)blocks), dim3(kBlockThreads), table_bytes, stream>>>(p);
  }
}

void launch_raw_set_bitmap(int key_bytes, int blocks, hipStream_t stream, const RawSetBitmapParams& p) {
  if (key_bytes == 4) {
    set_dynamic_lds(raw_set_bitmap_kernel<4>, p.table_bytes);
    raw_set_bitmap_kernel<4><<<dim3((unsigned)blocks), dim3(kBlockThreads), p.table_bytes, stream>>>(p);
  } else {
    set_dynamic_lds(raw_set_bitmap_kernel<8>, p.table_bytes);
    raw_set_bitmap_kernel<8><<<dim3((unsigned)blocks), dim3(kBlockThreads), p.table_bytes, stream>>>(p);
  }
}

int waves_scan_raw_set(int key_bytes) {
  static const int cap4 = max_waves_per_cu_lean(scan_raw_set_kernel<4>), cap8 = max_waves_per_cu_lean(scan_raw_set_kernel<8>);
  return key_bytes == 4 ? cap4 : cap8;
}
int waves_raw_set_bitmap(int key_bytes) {
  static const int cap4 = max_waves_per_cu_lean(raw_set_bitmap_kernel<4>), cap8 = max_waves_per_cu_lean(raw_set_bitmap_kernel<8>);
  return key_bytes == 4 ? cap4 : cap8;
}

}  // namespace pg
