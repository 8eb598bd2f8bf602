// Stand-alone check of the chunk codecs (pg_chunk_codec.h), for a sanitizer build on the CPU (make -C pinot_amd/csrc sanitize-chunk-codec): the
// edge corpus of the LZ4 block and Snappy raw formats decoded into exactly-sized heap buffers, every malformed chunk through the parsers the
// device kernel shares, and the chunk file's header / offset-table checks.  Exit status 0 and "ok" when every expectation holds.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../pg_chunk_codec.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using namespace pgcodec;
typedef std::vector<uint8_t> Bytes;

// A chunk under construction: the compressed bytes and, beside them, what they must decode to (built byte by byte, the definition of a match).
struct Chunk {
  Bytes z, raw;
  void literal_bytes(Bytes& to, uint32_t n) { for (uint32_t i = 0; i < n; ++i) { const uint8_t b = (uint8_t)(raw.size() * 7 + 3); to.push_back(b); raw.push_back(b); } }
  void match_bytes(uint32_t dist, uint32_t n) { for (uint32_t i = 0; i < n; ++i) raw.push_back(raw[raw.size() - dist]); }
  // LZ4: one sequence; match_len 0 = the block's last sequence (literals only)
  void lz4(uint32_t lit, uint32_t dist, uint32_t match_len) {
    const uint32_t ml = match_len ? match_len - 4 : 0;
    z.push_back((uint8_t)((lit < 15 ? lit : 15) << 4 | (ml < 15 ? ml : 15)));
    if (lit >= 15) { uint32_t r = lit - 15; while (r >= 255) { z.push_back(255); r -= 255; } z.push_back((uint8_t)r); }
    literal_bytes(z, lit);
    if (!match_len) return;
    z.push_back((uint8_t)dist); z.push_back((uint8_t)(dist >> 8));
    if (ml >= 15) { uint32_t r = ml - 15; while (r >= 255) { z.push_back(255); r -= 255; } z.push_back((uint8_t)r); }
    match_bytes(dist, match_len);
  }
  // Snappy elements (the varint goes in front at the end: snappy_done)
  void snappy_literal(uint32_t n, int extra_bytes = -1) {
    int nb = extra_bytes >= 0 ? extra_bytes : (n <= 60 ? 0 : n <= 256 ? 1 : n <= 65536 ? 2 : 3);
    if (nb == 0) z.push_back((uint8_t)((n - 1) << 2));
    else { z.push_back((uint8_t)((59 + nb) << 2)); for (int i = 0; i < nb; ++i) z.push_back((uint8_t)((n - 1) >> (8 * i))); }
    literal_bytes(z, n);
  }
  void snappy_copy1(uint32_t dist, uint32_t n) { z.push_back((uint8_t)(1 | (n - 4) << 2 | (dist >> 8) << 5)); z.push_back((uint8_t)dist); match_bytes(dist, n); }
  void snappy_copy2(uint32_t dist, uint32_t n) { z.push_back((uint8_t)(2 | (n - 1) << 2)); z.push_back((uint8_t)dist); z.push_back((uint8_t)(dist >> 8)); match_bytes(dist, n); }
  void snappy_copy4(uint32_t dist, uint32_t n) { z.push_back((uint8_t)(3 | (n - 1) << 2)); for (int i = 0; i < 4; ++i) z.push_back((uint8_t)(dist >> (8 * i))); match_bytes(dist, n); }
  void snappy_done() { Bytes v; uint32_t n = (uint32_t)raw.size(); while (n >= 128) { v.push_back((uint8_t)(n | 128)); n >>= 7; } v.push_back((uint8_t)n); z.insert(z.begin(), v.begin(), v.end()); }
};

// decodes into a heap buffer of exactly `expect` bytes, from a heap copy of exactly the compressed bytes
static int decode(int codec, const Bytes& z, uint32_t expect, Bytes* out = nullptr) {
  std::unique_ptr<uint8_t[]> src(new uint8_t[z.size() ? z.size() : 1]);
  if (!z.empty()) memcpy(src.get(), z.data(), z.size());
  std::unique_ptr<uint8_t[]> dst(new uint8_t[expect ? expect : 1]);
  const int r = decode_chunk_host(codec, src.get(), (uint32_t)z.size(), dst.get(), expect);
  if (out) out->assign(dst.get(), dst.get() + expect);
  return r;
}
static void good(int codec, const Chunk& c) {
  Bytes got;
  EXPECT(decode(codec, c.z, (uint32_t)c.raw.size(), &got) == kEnd);
  EXPECT(got == c.raw);
  // the same chunk against a size one short and one long: never kEnd
  EXPECT(decode(codec, c.z, (uint32_t)c.raw.size() + 1) != kEnd);
  if (!c.raw.empty()) EXPECT(decode(codec, c.z, (uint32_t)c.raw.size() - 1) != kEnd);
  // every proper prefix of the compressed bytes: an error, never a write outside the buffer
  for (size_t cut = 0; cut < c.z.size() && cut < 600; ++cut) EXPECT(decode(codec, Bytes(c.z.begin(), c.z.begin() + cut), (uint32_t)c.raw.size()) != kEnd);
}

static void lz4_corpus() {
  { Chunk c; c.lz4(8, 0, 0); good(kLz4, c); }                                              // literal-only block
  { Chunk c; c.lz4(4, 4, 8); c.lz4(0, 2, 5); c.lz4(5, 0, 0); good(kLz4, c); }              // an empty literal run before a match
  for (uint32_t lit : {14u, 15u, 270u, 271u, 15u + 255u * 3u}) { Chunk c; c.lz4(lit, lit, 4); c.lz4(5, 0, 0); good(kLz4, c); }      // token only, 15+0, 15+255+0, 15+255+1; distance == produced
  for (uint32_t ml : {4u, 18u, 19u, 274u, 275u, 1000u}) { Chunk c; c.lz4(40, 33, ml); c.lz4(6, 0, 0); good(kLz4, c); }
  for (uint32_t dist : {1u, 2u, 3u, 4u, 63u, 64u, 65u}) {
    for (uint32_t ml : {4u, dist + 1, dist * 64 + 70, 129u}) { Chunk c; c.lz4(dist + 2, dist, ml < 4 ? 4 : ml); c.lz4(5, 0, 0); good(kLz4, c); }      // longer than the distance by 1, and by more than 64 x
  }
  { Chunk c; c.raw.reserve(65536); c.z.push_back(0x1F); c.z.push_back(0); c.raw.push_back(0); c.z.push_back(1); c.z.push_back(0);      // 1 literal (zero), one long match at distance 1
    uint32_t ml = 65536 - 8 - 1 - 5, r = ml - 4 - 15; while (r >= 255) { c.z.push_back(255); r -= 255; } c.z.push_back((uint8_t)r); c.match_bytes(1, ml);
    c.z.push_back(0x50); for (int i = 0; i < 5; ++i) { c.z.push_back(0); c.raw.push_back(0); }
    EXPECT(c.raw.size() == 65536 - 8); good(kLz4, c); }
  { Chunk c; c.lz4(4000, 0, 0); EXPECT(c.z.size() > c.raw.size()); good(kLz4, c); }        // incompressible: larger than the raw chunk
}

static void snappy_corpus() {
  for (uint32_t n : {1u, 59u, 60u, 61u, 256u, 257u, 4000u}) { Chunk c; c.snappy_literal(n); c.snappy_done(); good(kSnappy, c); }      // tags 0..59, 60 (1 length byte), 61 (2)
  { Chunk c; c.snappy_literal(5, 3); c.snappy_literal(7, 4); c.snappy_done(); good(kSnappy, c); }      // tags 62 and 63 (3- and 4-byte lengths)
  for (uint32_t n : {4u, 11u}) { Chunk c; c.snappy_literal(300); c.snappy_copy1(299, n); c.snappy_copy1(300 + n, n); c.snappy_literal(1); c.snappy_done(); good(kSnappy, c); }      // copy-1, offsets above 255; distance == produced
  for (uint32_t dist : {1u, 2u, 3u, 4u, 63u, 64u, 65u}) { Chunk c; c.snappy_literal(dist + 1); c.snappy_copy1(dist, 5); c.snappy_copy2(dist, 64); c.snappy_copy2(dist, dist + 1 > 64 ? 64 : dist + 1); c.snappy_copy4(dist, 33); c.snappy_done(); good(kSnappy, c); }
  { Chunk c; c.snappy_literal(1); for (int i = 0; i < 70; ++i) c.snappy_copy2(1, 64); c.snappy_done(); good(kSnappy, c); }      // a run far longer than its distance
  { Chunk c; c.snappy_literal(3000); c.snappy_copy2(2999, 64); c.snappy_copy4(3000, 1); c.snappy_done(); good(kSnappy, c); }
  { Chunk c; c.snappy_done(); good(kSnappy, c); }                                          // the empty chunk: varint 0
}

static void malformed() {
  const uint8_t L = 0x40;      // LZ4 token: 4 literals, match length 4
  EXPECT(decode(kLz4, {L, 1, 2, 3, 4, 0, 0, 0x50, 1, 2, 3, 4, 5}, 13) == kErrBadDistance);                 // distance 0
  EXPECT(decode(kLz4, {L, 1, 2, 3, 4, 5, 0, 0x50, 1, 2, 3, 4, 5}, 13) == kErrBadDistance);                 // one beyond the produced bytes
  EXPECT(decode(kLz4, {L, 1, 2, 3, 4, 4, 0, 0x50, 1, 2, 3, 4, 5}, 13) == kEnd);                            // (the same block, well formed)
  EXPECT(decode(kLz4, {0x50, 1, 2, 3, 4}, 5) == kErrLiteralPastInput);                                     // a literal run one byte past the input
  EXPECT(decode(kLz4, {0xF0}, 600) == kErrTruncatedLength);                                                // a literal length chain cut by the chunk's end
  EXPECT(decode(kLz4, {0xF0, 255, 255}, 600) == kErrLiteralPastInput);                                     // ... and one that already promises more than the chunk holds
  EXPECT(decode(kLz4, {0x4F, 1, 2, 3, 4, 4, 0, 255}, 600) == kErrTruncatedLength);                         // a match length chain that never ends
  EXPECT(decode(kLz4, {L, 1, 2, 3, 4, 4}, 13) == kErrTruncatedOffset);                                     // half an offset
  EXPECT(decode(kLz4, {L, 1, 2, 3, 4, 4, 0, 0x50, 1, 2, 3, 4, 5}, 12) == kErrOutputOverrun);               // output one byte long
  EXPECT(decode(kLz4, {L, 1, 2, 3, 4, 4, 0, 0x50, 1, 2, 3, 4, 5}, 14) == kErrOutputShort);                 // output one byte short
  EXPECT(decode(kLz4, {L, 1, 2, 3, 4, 4, 0}, 7) == kErrOutputOverrun);                                     // a match past the expected size
  EXPECT(decode(kLz4, {L, 1, 2, 3, 4, 4, 0}, 9) == kErrOutputShort);                                       // a block that ends on a match, short of the size
  EXPECT(decode(kLz4, {}, 4) == kErrOutputShort);
  EXPECT(decode(kLz4, {0xF0, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 0}, 100000) == kErrLiteralPastInput);
  // Snappy: varint 8, literal of 4, copy-1 of 4 at distance d
  EXPECT(decode(kSnappy, {8, 3 << 2, 1, 2, 3, 4, 1, 4}, 8) == kEnd);
  EXPECT(decode(kSnappy, {8, 3 << 2, 1, 2, 3, 4, 1, 0}, 8) == kErrBadDistance);                            // distance 0
  EXPECT(decode(kSnappy, {8, 3 << 2, 1, 2, 3, 4, 1, 5}, 8) == kErrBadDistance);                            // one beyond the produced bytes
  EXPECT(decode(kSnappy, {8, 4 << 2, 1, 2, 3, 4}, 8) == kErrLiteralPastInput);                             // a literal run one byte past the input
  EXPECT(decode(kSnappy, {8, 61 << 2, 3}, 8) == kErrTruncatedLength);                                      // a 2-byte literal length cut after 1
  EXPECT(decode(kSnappy, {8, 3 << 2, 1, 2, 3, 4, 1}, 8) == kErrTruncatedOffset);                           // copy-1 without its offset byte
  EXPECT(decode(kSnappy, {8, 3 << 2, 1, 2, 3, 4, 2 | 3 << 2, 4}, 8) == kErrTruncatedOffset);               // copy-2 with half an offset
  EXPECT(decode(kSnappy, {8, 3 << 2, 1, 2, 3, 4, 3 | 3 << 2, 4, 0, 0}, 8) == kErrTruncatedOffset);         // copy-4 with three offset bytes
  EXPECT(decode(kSnappy, {7, 3 << 2, 1, 2, 3, 4, 1, 4}, 7) == kErrOutputOverrun);                          // output one byte long
  EXPECT(decode(kSnappy, {9, 3 << 2, 1, 2, 3, 4, 1, 4}, 9) == kErrOutputShort);                            // output one byte short
  EXPECT(decode(kSnappy, {9, 3 << 2, 1, 2, 3, 4, 1, 4}, 8) == kErrVarintMismatch);                         // a varint that disagrees with the header
  EXPECT(decode(kSnappy, {0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80, 0x80}, 8) == kErrVarint);              // a varint that never ends
  EXPECT(decode(kSnappy, {0x88, 0x80}, 8) == kErrVarint);                                                  // ... cut by the chunk's end
  EXPECT(decode(kSnappy, {0x88, 0x80, 0x80, 0x80, 0x10, 0}, 8) == kErrVarintMismatch);                     // 2^32 + 8 does not fit and does not match
  EXPECT(decode(kSnappy, {8, 63 << 2, 255, 255, 255, 255, 1}, 8) == kErrLiteralPastInput);                 // literal length 2^32
  EXPECT(decode(kSnappy, {}, 8) == kErrVarint);
  EXPECT(decode(2, {8, 3 << 2, 1, 2, 3, 4, 1, 4}, 8) == kErrCodec && decode(4, {0}, 0) == kErrCodec && decode(0, {0}, 0) == kErrCodec);
}

static void put32(Bytes& f, uint32_t v) { for (int s = 24; s >= 0; s -= 8) f.push_back((uint8_t)(v >> s)); }
// a chunk file of `version` over already-compressed chunks
static Bytes chunk_file(int version, int codec, int docs_per_chunk, int entry, int num_docs, const std::vector<Bytes>& chunks) {
  Bytes f;
  put32(f, (uint32_t)version); put32(f, (uint32_t)chunks.size()); put32(f, (uint32_t)docs_per_chunk); put32(f, (uint32_t)entry);
  if (version > 1) { put32(f, (uint32_t)num_docs); put32(f, (uint32_t)codec); put32(f, 28); }
  const int ob = version <= 2 ? 4 : 8;
  uint64_t at = f.size() + (uint64_t)ob * chunks.size();
  for (const Bytes& c : chunks) { if (ob == 8) put32(f, (uint32_t)(at >> 32)); put32(f, (uint32_t)at); at += c.size(); }
  for (const Bytes& c : chunks) f.insert(f.end(), c.begin(), c.end());
  return f;
}

static void files() {
  // 5 docs of 4 bytes in chunks of 2: chunks of 8, 8 and 4 bytes
  std::vector<Bytes> lz, sn;
  Bytes want;
  for (int c = 0; c < 3; ++c) {
    Chunk a, b;
    const uint32_t n = c < 2 ? 8 : 4;
    a.lz4(n, 0, 0); b.snappy_literal(n); b.snappy_done();
    lz.push_back(a.z); sn.push_back(b.z);
    want.insert(want.end(), a.raw.begin(), a.raw.end());
    EXPECT(a.raw == b.raw);
  }
  for (int version = 1; version <= 4; ++version) {
    for (int codec : {kLz4, kSnappy}) {
      if (version == 1 && codec == kLz4) continue;      // version 1 carries no codec field: always SNAPPY
      const Bytes f = chunk_file(version, codec, 2, 4, 5, codec == kLz4 ? lz : sn);
      ChunkFile cf;
      EXPECT(parse_chunk_header(f.data(), f.size(), &cf) == kFileOk && cf.codec == codec && cf.num_chunks == 3 && cf.offset_bytes == (version <= 2 ? 4 : 8));
      EXPECT(cf.header_start == (version == 1 ? 16u : 28u) && cf.data_start == cf.header_start + 3u * (unsigned)cf.offset_bytes);
      EXPECT(validate_chunk_table(cf, f.data(), f.size(), 5) == kFileOk);
      EXPECT(validate_chunk_table(cf, f.data(), f.size(), 4) == kFileBadChunkCount && validate_chunk_table(cf, f.data(), f.size(), 7) == kFileBadChunkCount);
      EXPECT(chunk_expect_bytes(cf, 5, 0) == 8 && chunk_expect_bytes(cf, 5, 2) == 4 && chunk_expect_bytes(cf, 6, 2) == 8);
      std::unique_ptr<uint8_t[]> out(new uint8_t[20]);
      int bad = -1;
      EXPECT(decode_file_host(cf, f.data(), f.size(), 5, out.get(), &bad) == kEnd && memcmp(out.get(), want.data(), 20) == 0);
      // the offset table: decreasing, past the file, into the table itself; the file cut inside the table
      const size_t second = (size_t)cf.header_start + (size_t)cf.offset_bytes * 2 - 1;      // the low byte of chunk 1's offset
      Bytes g = f; g[second] = (uint8_t)(g[second] - 20); EXPECT(validate_chunk_table(cf, g.data(), g.size(), 5) == kFileBadOffsets);
      g = f; g[second - 1] = 0x7F; EXPECT(validate_chunk_table(cf, g.data(), g.size(), 5) == kFileBadOffsets);
      g = f; g[(size_t)cf.header_start + (size_t)cf.offset_bytes - 1] = 0; EXPECT(validate_chunk_table(cf, g.data(), g.size(), 5) == kFileBadOffsets);
      EXPECT(validate_chunk_table(cf, f.data(), cf.data_start - 1, 5) == kFileTruncated);
      // a chunk that is malformed: the file decoder names it
      g = f; g.pop_back();
      EXPECT(decode_file_host(cf, g.data(), g.size(), 5, out.get(), &bad) != kEnd && bad == 2);
    }
  }
  ChunkFile cf;
  const Bytes tiny(12, 0);
  EXPECT(parse_chunk_header(tiny.data(), tiny.size(), &cf) == kFileTruncated);
  Bytes v9 = chunk_file(2, kLz4, 2, 4, 5, lz); v9[3] = 9;
  EXPECT(parse_chunk_header(v9.data(), v9.size(), &cf) == kFileOk && validate_chunk_table(cf, v9.data(), v9.size(), 5) == kFileBadHeader);
  Bytes cut = chunk_file(2, kLz4, 2, 4, 5, lz); cut.resize(20);
  EXPECT(parse_chunk_header(cut.data(), cut.size(), &cf) == kFileTruncated);
}

int main() {
  lz4_corpus();
  snappy_corpus();
  malformed();
  files();
  if (failures) { fprintf(stderr, "%d expectation(s) failed\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
