// pg_order_image.h -- the order-preserving 64-bit image of a raw column's value (pg_rank_image.h states the mapping): what the rank image's
// dictionary (pg_unit_rank_image.hip) and the value lists of PERCENTILE / DISTINCTCOUNT on raw columns (pg_scan_collect.h) are sorted by.
// Double.compare's order, every NaN the canonical one, FLOAT widened exactly; rank_image_value_bits (pg_rank_image.h) is the way back.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_device.h"

namespace pg {

__device__ __forceinline__ unsigned long long order_image_of_double_bits(unsigned long long b) {
  if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) b = 0x7FF8000000000000ull;      // every NaN is Double.NaN
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

__device__ __forceinline__ unsigned long long order_image(const uint8_t* __restrict__ raw, int vkind, long long doc) {
  if (vkind == kValI32) return (unsigned long long)(long long)(int32_t)__builtin_bswap32(reinterpret_cast<const uint32_t*>(raw)[doc]) ^ (1ull << 63);
  if (vkind == kValI64) return __builtin_bswap64(reinterpret_cast<const unsigned long long*>(raw)[doc]) ^ (1ull << 63);
  if (vkind == kValF32) {
    const float f = __uint_as_float(__builtin_bswap32(reinterpret_cast<const uint32_t*>(raw)[doc]));
    return order_image_of_double_bits((unsigned long long)__double_as_longlong((double)f));      // (float -> double is exact)
  }
  return order_image_of_double_bits(__builtin_bswap64(reinterpret_cast<const unsigned long long*>(raw)[doc]));
}

// The same images of values a kernel has already loaded with wide loads: `host` is the value in host byte order (the stored bytes swapped).
__device__ __forceinline__ unsigned long long order_image_of_host32(int vkind, uint32_t host) {
  if (vkind == kValF32) return order_image_of_double_bits((unsigned long long)__double_as_longlong((double)__uint_as_float(host)));
  return (unsigned long long)(long long)(int32_t)host ^ (1ull << 63);
}
__device__ __forceinline__ unsigned long long order_image_of_host64(int vkind, unsigned long long host) {
  return vkind == kValI64 ? host ^ (1ull << 63) : order_image_of_double_bits(host);
}

}  // namespace pg
