// Chunk-compressed raw forward indexes (FixedByteChunkSVForwardIndexReader over BaseChunkForwardIndexReader): the file layout, and the two
// byte-oriented LZ77 codecs the fixed-byte writers produce by default -- LZ4 block format (ChunkCompressionType.LZ4 = 3: a chunk is ONE bare
// block, no frame, no length prefix) and Snappy raw format (SNAPPY = 1, and every version-1 file: a varint length, then literal / copy-1 /
// copy-2 / copy-4 elements).  Neither has an entropy stage, so neither needs a library.
//
// Plain C++ that compiles for the host and for the device.  A parser step returns an error or ONE VALIDATED SEQUENCE: a literal run (offset
// into the chunk's compressed bytes, length) followed by a match (distance, length); either half may be empty.  Every bound is checked in the
// parser -- the copy loops of decode_chunk_host below and of chunk_decode_kernel (pg_chunk_decode.h) execute only what a step returned, so
// the bounds logic lives once and is checked on the CPU (host/check/chunk_codec_main.cpp under AddressSanitizer + UBSan).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PG_CODEC_HD __host__ __device__ inline
#else
#define PG_CODEC_HD inline
#endif

namespace pgcodec {

// ChunkCompressionType.getValue()
enum : int { kPassThrough = 0, kSnappy = 1, kZstandard = 2, kLz4 = 3, kLz4LengthPrefixed = 4, kGzip = 5 };

inline const char* codec_name(int c) {
  switch (c) {
    case kPassThrough: return "PASS_THROUGH";
    case kSnappy: return "SNAPPY";
    case kZstandard: return "ZSTANDARD";
    case kLz4: return "LZ4";
    case kLz4LengthPrefixed: return "LZ4_LENGTH_PREFIXED";
    case kGzip: return "GZIP";
    default: return "unknown";
  }
}

// Parser results.  0: `seq` holds the next sequence; kEnd: the chunk ended and produced exactly the expected bytes; anything else: malformed.
enum : int {
  kSeq = 0,
  kEnd = 1,
  kErrTruncatedLength = 2,    // a length chain or a tag's length bytes run past the chunk
  kErrLiteralPastInput = 3,   // a literal run does not lie inside the chunk's compressed bytes
  kErrOutputOverrun = 4,      // literals plus match exceed the expected decompressed size
  kErrTruncatedOffset = 5,    // a match offset runs past the chunk
  kErrBadDistance = 6,        // distance 0, or beyond the bytes produced so far
  kErrOutputShort = 7,        // the chunk ended before the expected size
  kErrVarint = 8,             // Snappy: the length preamble never ends, or does not fit 32 bits
  kErrVarintMismatch = 9,     // Snappy: the length preamble is not the expected size
  kErrCodec = 10              // not a codec this file decodes
};

struct Sequence {
  uint32_t lit_off;     // literal run: [lit_off, lit_off + lit_len) of the chunk's compressed bytes
  uint32_t lit_len;
  uint32_t distance;    // match: out[d + i] = out[d - distance + (i mod distance)] for i < match_len, d = bytes produced after the literals
  uint32_t match_len;   // 0: no match (distance is 0 then)
};

// The walk over one chunk.  `produced` counts the bytes of every sequence returned so far.
struct Parser {
  const uint8_t* src;
  uint32_t n;           // compressed bytes of the chunk
  uint32_t ip;          // cursor
  uint32_t produced;
  uint32_t expect;      // decompressed size the header implies
};

PG_CODEC_HD void parser_init(Parser& p, const uint8_t* src, uint32_t n, uint32_t expect) { p.src = src; p.n = n; p.ip = 0; p.produced = 0; p.expect = expect; }

// LZ4 block: token (literal length << 4 | match length - 4), [length bytes], literals, then -- unless the block ends here -- a 2-byte
// little-endian offset and [length bytes].  The block ends after a literal run.
PG_CODEC_HD int lz4_next(Parser& p, Sequence& s) {
  s.lit_off = 0; s.lit_len = 0; s.distance = 0; s.match_len = 0;
  if (p.ip >= p.n) return p.produced == p.expect ? kEnd : kErrOutputShort;
  const uint32_t token = p.src[p.ip++];
  uint32_t lit = token >> 4;
  if (lit == 15) {
    for (;;) {
      if (p.ip >= p.n) return kErrTruncatedLength;
      const uint32_t b = p.src[p.ip++];
      lit += b;
      if (lit > p.n) return kErrLiteralPastInput;        // (also keeps the sum far from 2^32)
      if (b != 255) break;
    }
  }
  if (lit > p.n - p.ip) return kErrLiteralPastInput;
  if (lit > p.expect - p.produced) return kErrOutputOverrun;
  s.lit_off = p.ip; s.lit_len = lit;
  p.ip += lit; p.produced += lit;
  if (p.ip == p.n) return p.produced == p.expect ? kSeq : kErrOutputShort;      // the last sequence: literals only (kEnd comes on the next step)
  if (p.n - p.ip < 2) return kErrTruncatedOffset;
  const uint32_t dist = (uint32_t)p.src[p.ip] | ((uint32_t)p.src[p.ip + 1] << 8);
  p.ip += 2;
  if (dist == 0 || dist > p.produced) return kErrBadDistance;
  uint32_t ml = token & 15;
  if (ml == 15) {
    for (;;) {
      if (p.ip >= p.n) return kErrTruncatedLength;
      const uint32_t b = p.src[p.ip++];
      ml += b;
      if (ml > p.expect) return kErrOutputOverrun;
      if (b != 255) break;
    }
  }
  ml += 4;      // MINMATCH
  if (ml > p.expect - p.produced) return kErrOutputOverrun;
  s.distance = dist; s.match_len = ml;
  p.produced += ml;
  return kSeq;
}

// Snappy raw format: varint32 uncompressed length, then elements by tag & 3 -- 0: literal (length - 1 in the tag's upper six bits, 60..63: in
// the next 1..4 bytes), 1: copy with a 1-byte offset (length 4..11, offset 11 bits), 2: copy with a 2-byte offset, 3: copy with a 4-byte offset.
PG_CODEC_HD int snappy_next(Parser& p, Sequence& s) {
  s.lit_off = 0; s.lit_len = 0; s.distance = 0; s.match_len = 0;
  if (p.ip == 0) {
    uint64_t v = 0;
    int shift = 0;
    for (;;) {
      if (p.ip >= p.n || shift > 28) return kErrVarint;
      const uint32_t b = p.src[p.ip++];
      v |= (uint64_t)(b & 127) << shift;
      if (!(b & 128)) break;
      shift += 7;
    }
    if (v != (uint64_t)p.expect) return kErrVarintMismatch;
  }
  if (p.ip >= p.n) return p.produced == p.expect ? kEnd : kErrOutputShort;
  const uint32_t tag = p.src[p.ip++];
  const uint32_t kind = tag & 3;
  if (kind == 0) {
    uint64_t len = (tag >> 2);
    if (len >= 60) {
      const uint32_t nb = (uint32_t)len - 59;
      if (p.n - p.ip < nb) return kErrTruncatedLength;
      len = 0;
      for (uint32_t i = 0; i < nb; ++i) len |= (uint64_t)p.src[p.ip + i] << (8 * i);
      p.ip += nb;
    }
    len += 1;
    if (len > (uint64_t)(p.n - p.ip)) return kErrLiteralPastInput;
    if (len > (uint64_t)(p.expect - p.produced)) return kErrOutputOverrun;
    s.lit_off = p.ip; s.lit_len = (uint32_t)len;
    p.ip += (uint32_t)len; p.produced += (uint32_t)len;
    return kSeq;
  }
  uint32_t len, dist;
  if (kind == 1) {
    if (p.n - p.ip < 1) return kErrTruncatedOffset;
    len = 4 + ((tag >> 2) & 7);
    dist = ((tag >> 5) << 8) | (uint32_t)p.src[p.ip];
    p.ip += 1;
  } else if (kind == 2) {
    if (p.n - p.ip < 2) return kErrTruncatedOffset;
    len = (tag >> 2) + 1;
    dist = (uint32_t)p.src[p.ip] | ((uint32_t)p.src[p.ip + 1] << 8);
    p.ip += 2;
  } else {
    if (p.n - p.ip < 4) return kErrTruncatedOffset;
    len = (tag >> 2) + 1;
    dist = (uint32_t)p.src[p.ip] | ((uint32_t)p.src[p.ip + 1] << 8) | ((uint32_t)p.src[p.ip + 2] << 16) | ((uint32_t)p.src[p.ip + 3] << 24);
    p.ip += 4;
  }
  if (dist == 0 || dist > p.produced) return kErrBadDistance;
  if (len > p.expect - p.produced) return kErrOutputOverrun;
  s.distance = dist; s.match_len = len;
  p.produced += len;
  return kSeq;
}

template <int CODEC>
PG_CODEC_HD int next_sequence(Parser& p, Sequence& s) {
  if (CODEC == kLz4) return lz4_next(p, s);
  return snappy_next(p, s);
}

// The host decoder: `dst` has exactly `expect` bytes.  Returns kEnd, or the parser's error (dst then holds a prefix of the chunk and nothing
// was written outside it).
template <int CODEC>
inline int decode_chunk_host_as(const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t expect) {
  Parser p;
  parser_init(p, src, n, expect);
  uint32_t d = 0;
  for (;;) {
    Sequence s;
    const int r = next_sequence<CODEC>(p, s);
    if (r != kSeq) return r;
    if (s.lit_len) memcpy(dst + d, src + s.lit_off, s.lit_len);
    d += s.lit_len;
    for (uint32_t i = 0; i < s.match_len; ++i) dst[d + i] = dst[d - s.distance + i];      // byte by byte: an overlapping match repeats its period
    d += s.match_len;
  }
}

inline int decode_chunk_host(int codec, const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t expect) {
  if (codec == kLz4) return decode_chunk_host_as<kLz4>(src, n, dst, expect);
  if (codec == kSnappy) return decode_chunk_host_as<kSnappy>(src, n, dst, expect);
  return kErrCodec;
}

// ---- the file ----
// BaseChunkForwardIndexWriter.writeHeader: big-endian ints version, numChunks, numDocsPerChunk, sizeOfEntry, and from version 2 on totalDocs,
// compressionType, dataHeaderStart; then numChunks chunk offsets (absolute file positions; 4 bytes in versions 1 and 2, 8 bytes in 3 and 4),
// then the chunks.  Version 1 has the 16-byte header only (its codec is SNAPPY: BaseChunkForwardIndexReader.java:92-95); version 4
// (FixedBytePower2ChunkSVForwardIndexReader) is version 3 with a power-of-two numDocsPerChunk.
struct ChunkFile {
  int version, num_chunks, docs_per_chunk, entry_size, codec;
  uint64_t header_start;    // of the offset table
  int offset_bytes;         // 4 or 8
  uint64_t data_start;      // end of the offset table
};

enum : int { kFileOk = 0, kFileTruncated = 1, kFileBadHeader = 2, kFileBadChunkCount = 3, kFileBadOffsets = 4 };

inline uint32_t be32_at(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
inline uint64_t be64_at(const uint8_t* p) { return ((uint64_t)be32_at(p) << 32) | (uint64_t)be32_at(p + 4); }

// Header only: what every raw column needs (PASS_THROUGH ones included; the version is judged where chunks are decoded: validate_chunk_table).
inline int parse_chunk_header(const uint8_t* file, uint64_t size, ChunkFile* out) {
  if (size < 16) return kFileTruncated;
  ChunkFile f;
  f.version = (int)be32_at(file);
  f.num_chunks = (int)be32_at(file + 4);
  f.docs_per_chunk = (int)be32_at(file + 8);
  f.entry_size = (int)be32_at(file + 12);
  f.codec = kSnappy;
  f.header_start = 16;
  if (f.version > 1) {
    if (size < 28) return kFileTruncated;
    f.codec = (int)be32_at(file + 20);
    f.header_start = (uint64_t)be32_at(file + 24);
  }
  f.offset_bytes = f.version <= 2 ? 4 : 8;
  if (f.num_chunks < 0 || f.docs_per_chunk < 0 || f.entry_size < 0) return kFileBadHeader;
  f.data_start = f.header_start + (uint64_t)f.num_chunks * (uint64_t)f.offset_bytes;
  *out = f;
  return kFileOk;
}

inline uint64_t chunk_offset(const ChunkFile& f, const uint8_t* file, int chunk) {
  const uint8_t* p = file + f.header_start + (uint64_t)chunk * (uint64_t)f.offset_bytes;
  return f.offset_bytes == 4 ? (uint64_t)be32_at(p) : be64_at(p);
}

// What a compressed file must satisfy before any chunk is decoded: a version from 1 to 4, numChunks consistent with numDocs and numDocsPerChunk, the offset table
// inside the file, offsets monotonic, inside the file and behind the table, every extent below 2^31 bytes.
inline int validate_chunk_table(const ChunkFile& f, const uint8_t* file, uint64_t size, int64_t num_docs) {
  if (f.version < 1 || f.version > 4) return kFileBadHeader;
  if (f.docs_per_chunk < 1 || f.entry_size < 1 || num_docs < 1) return kFileBadHeader;
  if ((uint64_t)f.docs_per_chunk * (uint64_t)f.entry_size >= (1ull << 31)) return kFileBadHeader;
  if ((int64_t)f.num_chunks != (num_docs + f.docs_per_chunk - 1) / f.docs_per_chunk) return kFileBadChunkCount;
  if (f.header_start < (f.version > 1 ? 28u : 16u) || f.header_start > size || f.data_start > size) return kFileTruncated;
  uint64_t prev = f.data_start;
  for (int c = 0; c < f.num_chunks; ++c) {
    const uint64_t o = chunk_offset(f, file, c);
    if (o < prev || o > size) return kFileBadOffsets;
    if (c > 0 && o - prev >= (1ull << 31)) return kFileBadOffsets;
    prev = o;
  }
  if (size - prev >= (1ull << 31)) return kFileBadOffsets;
  return kFileOk;
}

// The decompressed size of chunk c: the writer compresses only what was written (BaseChunkForwardIndexWriter.writeChunk).
inline uint64_t chunk_expect_bytes(const ChunkFile& f, int64_t num_docs, int chunk) {
  const int64_t docs = chunk + 1 < f.num_chunks ? f.docs_per_chunk : num_docs - (int64_t)(f.num_chunks - 1) * f.docs_per_chunk;
  return (uint64_t)docs * (uint64_t)f.entry_size;
}

// Every chunk of a validated file into `dst` (num_docs * entry_size bytes, dense, big-endian as stored).  Returns kEnd; on an error the
// parser's code with *bad_chunk set.
inline int decode_file_host(const ChunkFile& f, const uint8_t* file, uint64_t size, int64_t num_docs, uint8_t* dst, int* bad_chunk) {
  for (int c = 0; c < f.num_chunks; ++c) {
    const uint64_t o = chunk_offset(f, file, c);
    const uint64_t end = c + 1 < f.num_chunks ? chunk_offset(f, file, c + 1) : size;
    const int r = decode_chunk_host(f.codec, file + o, (uint32_t)(end - o), dst + (uint64_t)c * (uint64_t)f.docs_per_chunk * (uint64_t)f.entry_size,
                                    (uint32_t)chunk_expect_bytes(f, num_docs, c));
    if (r != kEnd) { if (bad_chunk) *bad_chunk = c; return r; }
  }
  return kEnd;
}

}  // namespace pgcodec
