// The membership table of a PG_PRED_RAW_SET leaf (IN / NOT IN on a raw column): what the host builds and the kernels of pg_scan_raw_set.h
// probe in LDS.  Plain C++ (no HIP): the engine, the kernels and the host library's self-test all include it.
//
// Layout: `buckets` (a power of two) buckets of FOUR key slots.  4-byte keys (INT columns; FLOAT columns as float bit patterns): a bucket
// is 16 bytes, one ds_read_b128; 8-byte keys (LONG; DOUBLE as bit patterns): 32 bytes, two.  The builder retries hash multipliers (and
// doubles `buckets`) until EVERY key sits in its home bucket, so a lookup is one fixed, branch-free probe: read the bucket, compare four
// slots.  Slots no key claimed hold a COPY of a member key (the bucket's own first key, or the list's first key in an empty bucket): no
// value is stolen as an "empty" sentinel, so -1, 0 and INT_MIN are ordinary members.
//
// Keys are stored in the column's ON-DISK byte order as the kernels load it: a raw column is big-endian, a lane's little-endian dword load
// sees bswap32(value), and membership does not care -- the kernels hash and compare the loaded words without swapping every doc.  For
// 8-byte keys word 0 is the dword at the lower address (the swapped HIGH half of the value), word 1 the next.
//
// Sizing: with n keys thrown at B buckets the chance that some bucket gets five is about C(n, 5) / B^4; B = 2 n (at least 16) leaves a
// multiplier succeeding within a few tries (n = 1024, B = 2048: ~0.6 per try), a 32 KiB table for 1024 INT keys and 64 KiB for LONG keys.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define PG_RS_HD __host__ __device__ inline
#else
#define PG_RS_HD inline
#endif

namespace pg {

constexpr int kRawSetMaxValues = 1024;        // distinct values of one list (PG_RAW_SET_MAX_VALUES)
constexpr int kRawSetSlots = 4;               // key slots per bucket
constexpr int kRawSetMaxTableBytes = 64 * 1024;   // 4096 buckets of 4-byte keys, 2048 of 8-byte keys: the builder gives up beyond (never seen: see the sizing note);
                                                  // two workgroups' tables and their reduction records fit a CU's 160 KiB of LDS

// bucket of a 4-byte key (the dword as loaded); `shift` = 32 - log2(buckets)
PG_RS_HD uint32_t raw_set_bucket32(uint32_t w, uint32_t mult, uint32_t shift) {
  uint32_t x = w * mult;
  x ^= x >> 15;
  x *= 0x9E3779B1u;
  return shift >= 32u ? 0u : x >> shift;
}
// bucket of an 8-byte key (its two dwords as loaded)
PG_RS_HD uint32_t raw_set_bucket64(uint32_t w0, uint32_t w1, uint32_t mult, uint32_t shift) {
  uint32_t x = w0 * mult + w1 * (mult ^ 0x5BD1E994u);      // (mult is odd, so is mult ^ an even constant)
  x ^= x >> 15;
  x *= 0x9E3779B1u;
  x ^= w1 >> 7;
  x *= 0x85EBCA6Bu;
  return shift >= 32u ? 0u : x >> shift;
}

struct RawSetTable {
  int key_bytes = 4;                 // 4 or 8
  uint32_t buckets = 0, mult = 1, shift = 32;
  std::vector<uint32_t> words;       // buckets * kRawSetSlots keys, key_bytes each
  size_t bytes() const { return words.size() * 4; }
};

inline uint32_t raw_set_bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }
// the key as the kernels load it from a big-endian column
inline uint32_t raw_set_disk_key32(uint32_t value_bits) { return raw_set_bswap32(value_bits); }
inline void raw_set_disk_key64(uint64_t value_bits, uint32_t* w0, uint32_t* w1) {
  *w0 = raw_set_bswap32((uint32_t)(value_bits >> 32));
  *w1 = raw_set_bswap32((uint32_t)value_bits);
}

// `keys`: the distinct member values' bit patterns (int32 / float bits in the low half for key_bytes == 4), at least one, at most
// kRawSetMaxValues.  False: no multiplier placed every key within kRawSetMaxTableBytes.
inline bool build_raw_set_table(const std::vector<uint64_t>& keys, int key_bytes, RawSetTable* t) {
  const size_t n = keys.size();
  if (n == 0 || n > (size_t)kRawSetMaxValues || (key_bytes != 4 && key_bytes != 8)) return false;
  uint32_t buckets = 16;
  while (buckets < 2 * n) buckets <<= 1;
  const int per_key = key_bytes / 4;
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  std::vector<uint8_t> fill;
  for (; (size_t)buckets * kRawSetSlots * key_bytes <= (size_t)kRawSetMaxTableBytes; buckets <<= 1) {
    uint32_t log2b = 0;
    while ((1u << log2b) < buckets) log2b++;
    const uint32_t shift = 32u - log2b;
    for (int attempt = 0; attempt < 64; ++attempt) {
      rng = rng * 6364136223846793005ull + 1442695040888963407ull;
      const uint32_t mult = (uint32_t)(rng >> 32) | 1u;
      fill.assign(buckets, 0);
      t->words.assign((size_t)buckets * kRawSetSlots * per_key, 0u);
      bool ok = true;
      for (size_t i = 0; i < n && ok; ++i) {
        uint32_t w0, w1 = 0, b;
        if (key_bytes == 4) { w0 = raw_set_disk_key32((uint32_t)keys[i]); b = raw_set_bucket32(w0, mult, shift); }
        else { raw_set_disk_key64(keys[i], &w0, &w1); b = raw_set_bucket64(w0, w1, mult, shift); }
        if (fill[b] == kRawSetSlots) { ok = false; break; }
        uint32_t* slot = t->words.data() + ((size_t)b * kRawSetSlots + fill[b]) * per_key;
        slot[0] = w0;
        if (per_key == 2) slot[1] = w1;
        fill[b]++;
      }
      if (!ok) continue;
      // unclaimed slots: a copy of a member (the bucket's first key; an empty bucket takes the list's first key)
      uint32_t any0, any1 = 0;
      if (key_bytes == 4) any0 = raw_set_disk_key32((uint32_t)keys[0]);
      else raw_set_disk_key64(keys[0], &any0, &any1);
      for (uint32_t b = 0; b < buckets; ++b) {
        uint32_t* bucket = t->words.data() + (size_t)b * kRawSetSlots * per_key;
        const uint32_t f0 = fill[b] ? bucket[0] : any0, f1 = fill[b] ? (per_key == 2 ? bucket[1] : 0u) : any1;
        for (int s = fill[b]; s < kRawSetSlots; ++s) {
          bucket[s * per_key] = f0;
          if (per_key == 2) bucket[s * per_key + 1] = f1;
        }
      }
      t->key_bytes = key_bytes; t->buckets = buckets; t->mult = mult; t->shift = shift;
      return true;
    }
  }
  return false;
}

// the probe the kernels run, on the host (tests; the value's bit pattern in, not the disk form)
inline bool raw_set_table_contains(const RawSetTable& t, uint64_t value_bits) {
  if (t.key_bytes == 4) {
    const uint32_t w = raw_set_disk_key32((uint32_t)value_bits);
    const uint32_t* bucket = t.words.data() + (size_t)raw_set_bucket32(w, t.mult, t.shift) * kRawSetSlots;
    return bucket[0] == w || bucket[1] == w || bucket[2] == w || bucket[3] == w;
  }
  uint32_t w0, w1;
  raw_set_disk_key64(value_bits, &w0, &w1);
  const uint32_t* bucket = t.words.data() + (size_t)raw_set_bucket64(w0, w1, t.mult, t.shift) * kRawSetSlots * 2;
  bool hit = false;
  for (int s = 0; s < kRawSetSlots; ++s) hit |= bucket[2 * s] == w0 && bucket[2 * s + 1] == w1;
  return hit;
}

// What a PG_PRED_RAW_SET list means for a column of `stored_type` (pg_data_type: 0 INT, 1 LONG, 2 FLOAT, 3 DOUBLE): the distinct member
// bit patterns, ascending as unsigned patterns.  Returns 0 ok; 1 the list holds a zero or a NaN (FLOAT / DOUBLE: declined); 2 more than
// kRawSetMaxValues distinct members.  `words`: two per value, low word first (int64 value, or the bits of the value as a double).
inline int decode_raw_set_words(int stored_type, const uint32_t* words, int num_words, std::vector<uint64_t>* keys) {
  keys->clear();
  for (int i = 0; i + 1 < num_words; i += 2) {
    const uint64_t v = (uint64_t)words[i] | ((uint64_t)words[i + 1] << 32);
    if (stored_type == 0) {
      const int64_t s = (int64_t)v;
      if (s < INT32_MIN || s > INT32_MAX) continue;            // can never equal an int
      keys->push_back((uint64_t)(uint32_t)(int32_t)s);
    } else if (stored_type == 1) {
      keys->push_back(v);
    } else {
      double d;
      memcpy(&d, &v, 8);
      if (d != d || d == 0.0) return 1;
      if (stored_type == 2) {
        const float f = (float)d;
        if ((double)f != d) continue;                          // not exactly a float: can never equal a float value
        uint32_t fb;
        memcpy(&fb, &f, 4);
        keys->push_back((uint64_t)fb);
      } else {
        keys->push_back(v);
      }
    }
  }
  std::sort(keys->begin(), keys->end());
  keys->erase(std::unique(keys->begin(), keys->end()), keys->end());
  return keys->size() > (size_t)kRawSetMaxValues ? 2 : 0;
}

}  // namespace pg
