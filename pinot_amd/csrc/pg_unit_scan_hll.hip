// Instantiates scan_hll_kernel, group_hll_kernel, hll_fold_kernel and hll_pack_kernel: DISTINCTCOUNTHLL's registers -- see pg_launch.h.
#include "pg_scan_hll.h"
#include "pg_launch.h"

namespace pg {

void launch_scan_hll(int blocks, size_t lds, hipStream_t stream, const HllParams& hp) {
  set_dynamic_lds(scan_hll_kernel, lds);
  scan_hll_kernel<<<dim3((unsigned)blocks), dim3(kHistBlockThreads), lds, stream>>>(hp);
}

int waves_scan_hll() {
  static const int cap = max_waves_per_cu(scan_hll_kernel);
  return cap;
}

void launch_group_hll(int blocks, size_t lds, hipStream_t stream, const HllParams& hp) {
  group_hll_kernel<<<dim3((unsigned)blocks), dim3(kDistinctBlockThreads), lds, stream>>>(hp);
}

int waves_group_hll() {
  static const int cap = max_waves_per_cu(group_hll_kernel);
  return cap;
}

void launch_hll_fold(long long rows, hipStream_t stream, HllFoldParams fp) {
  // a workgroup per 8192 dictIds of a row (at most 64 per row): the registers are merged into the row with atomics, so chunks of one row may overlap in time
  fp.words_per_chunk = 256;
  fp.chunks = std::max(1, std::min(64, (fp.words + fp.words_per_chunk - 1) / fp.words_per_chunk));
  fp.words_per_chunk = (fp.words + fp.chunks - 1) / fp.chunks;
  const size_t lds = (size_t)4 << fp.log2m;
  set_dynamic_lds(hll_fold_kernel, lds);
  hll_fold_kernel<<<dim3((unsigned)(rows * fp.chunks)), dim3(kHllFoldThreads), lds, stream>>>(fp);
}

void launch_hll_pack(const uint32_t* words, uint8_t* bytes, unsigned long long n, int num_cus, hipStream_t stream) {
  const unsigned long long n4 = n / 4;
  const unsigned blocks = (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>((n4 + 255) / 256, (unsigned long long)num_cus * 8));
  hll_pack_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(words, reinterpret_cast<uint32_t*>(bytes), n4);
}

}  // namespace pg
