// pg_hll.h -- the arithmetic of DISTINCTCOUNTHLL, shared by host and device code.
//
// What it restates: the HyperLogLog sketch DistinctCountHLLAggregationFunction.java builds through offer(Object) -- a 32-bit Murmur2 hash of
// the value as a long, 2^log2m registers of one rank each, the classic estimator with the linear-counting branch for small cardinalities.
// Everything here is integer arithmetic except hll_cardinality, which only the host calls.
//
// Pinned by the reference's goldens (InterSegmentAggregationSingleValueQueriesTest.testDistinctCountHLL): the INT hash, the index / rank rule
// at log2m = 8 and the estimator's default branch.  NOT pinned by anything here -- written from the published algorithm and to be looked at
// first in a parity run against a JVM: the high-word step of hll_hash_long, the boxing rules for LONG / FLOAT / DOUBLE, the alpha constants of
// log2m 4..6 and the linear-counting branch.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PG_HLL_FN __host__ __device__ __forceinline__
#else
#define PG_HLL_FN inline
#endif

namespace pg {

constexpr int kHllMinLog2m = 4, kHllMaxLog2m = 14, kHllDefaultLog2m = 8;
constexpr int kHllFunction = 7;      // PG_AGG_DISTINCTCOUNTHLL: the low byte of pg_aggregation.function; log2m travels in the bits above it

// log2m of a function word (PG_AGG_HLL(log2m)); the plain enumerator means the default.
PG_HLL_FN int hll_log2m_of(int32_t function) { const int v = (int)((uint32_t)function >> 8); return v == 0 ? kHllDefaultLog2m : v; }

// MurmurHash.hashLong: Murmur2 over the two 32-bit halves of the long, seed 0, all in wrapping 32-bit arithmetic.
PG_HLL_FN uint32_t hll_hash_long(uint64_t data) {
  const uint32_t M = 0x5bd1e995u;
  uint32_t h = 0u;
  uint32_t k = (uint32_t)data * M;
  k ^= k >> 24;
  h ^= k * M;
  k = (uint32_t)(data >> 32) * M;
  k ^= k >> 24;
  h *= M;
  h ^= k * M;
  h ^= h >> 13;
  h *= M;
  h ^= h >> 15;
  return h;
}

// Which long offer(Object) hashes, from the value as stored: INT sign-extended, LONG itself, FLOAT floatToRawIntBits sign-extended (the 32
// stored bits, not the float widened to a double), DOUBLE doubleToRawLongBits.  -0.0 and 0.0 differ, NaN payloads are kept.
PG_HLL_FN uint64_t hll_long_of_bits32(uint32_t stored) { return (uint64_t)(int64_t)(int32_t)stored; }      // INT and FLOAT alike

// The 32 stored bits of a FLOAT dictionary entry that was widened to a double (exactly, so narrowing restores it).  A NaN is narrowed by its
// bits: a conversion instruction may not keep the payload.
PG_HLL_FN uint32_t hll_float_bits_of_widened(uint64_t double_bits) {
  if ((double_bits & 0x7FF0000000000000ull) == 0x7FF0000000000000ull && (double_bits & 0x000FFFFFFFFFFFFFull) != 0ull)
    return (uint32_t)((double_bits >> 32) & 0x80000000ull) | 0x7F800000u | (uint32_t)((double_bits >> 29) & 0x007FFFFFull);
  double d;
  __builtin_memcpy(&d, &double_bits, 8);
  const float f = (float)d;
  uint32_t bits;
  __builtin_memcpy(&bits, &f, 4);
  return bits;
}

// The register a hash updates and the rank it offers: a rank is at most 32 - log2m + 1, so a register fits a byte.
PG_HLL_FN uint32_t hll_index(uint32_t x, int log2m) { return x >> (32 - log2m); }
PG_HLL_FN uint32_t hll_rank(uint32_t x, int log2m) {
  const uint32_t w = (x << log2m) | ((1u << (log2m - 1)) + 1u);      // (never zero: bit 0 is set)
  return (uint32_t)__builtin_clz(w) + 1u;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The estimate of a register set (host only).  Math.round is floor(x + 0.5), not banker's rounding.
inline int64_t hll_cardinality(const uint8_t* registers, int log2m) {
  const double m = (double)(1 << log2m);
  double alpha_mm;
  switch (log2m) {
    case 4: alpha_mm = 0.673 * m * m; break;
    case 5: alpha_mm = 0.697 * m * m; break;
    case 6: alpha_mm = 0.709 * m * m; break;
    default: alpha_mm = (0.7213 / (1.0 + 1.079 / m)) * m * m; break;
  }
  double sum = 0.0;
  int zeros = 0;
  for (int j = 0; j < (1 << log2m); ++j) {
    sum += 1.0 / (double)(1ull << registers[j]);
    zeros += registers[j] == 0;
  }
  const double estimate = alpha_mm / sum;
  if (estimate <= 2.5 * m) {
    // linear counting.  No zero register with so small an estimate (every register 1 gives 1.44 m): m ln(m / 0) is +Infinity, which
    // Math.round turns into Long.MAX_VALUE.
    if (zeros == 0) return INT64_MAX;
    return (int64_t)floor(m * log(m / (double)zeros) + 0.5);
  }
  return (int64_t)floor(estimate + 0.5);
}
#endif

}  // namespace pg
