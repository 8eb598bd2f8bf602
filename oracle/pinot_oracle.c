/*
 * pinot_oracle.c -- CPU restatement of the reference's per-segment scan -> filter -> aggregate path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under pinot_amd/ may include, link, load or call this file; it is
 * used by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg as the checker / CPU baseline.
 *
 * The reference (y-scope/pinot, Java) cannot be compiled in this environment (no JDK), so this file
 * restates the algorithms, function by function, each citing the reference file:line it follows.
 * Paths are under /root/reference with
 *   segl/ = pinot-segment-local/src/main/java/org/apache/pinot/segment/local/
 *   core/ = pinot-core/src/main/java/org/apache/pinot/core/
 *   sspi/ = pinot-segment-spi/src/main/java/org/apache/pinot/segment/spi/
 *
 * Parity pins: query-level results are pinned by the reference's own golden vectors over
 * test_data-sv.avro (tests/golden/, InnerSegmentAggregationSingleValueQueriesTest.java:44-112); the fixed-bit
 * forward-index and dictionary BYTE layouts are pinned by files the reference's own Java writers produced
 * (pinot-core/src/test/resources/data/paddingOld.tar.gz -> tests/golden/pinot_v1_segment_paddingOld.json: the
 * writer restatement reproduces them byte for byte) plus known-answer bytes derived from
 * PinotDataBitSet.writeInt; the raw chunk layout by its header fields.  RoaringBitmap (third-party
 * org.roaringbitmap:RoaringBitmap:1.3.0, not under /root/reference) follows the public RoaringFormatSpec:
 * serialized-byte parity is "unpinned", set semantics are pinned through the golden queries.  The iterator objects behind
 * numEntriesScannedInFilter are pinned by the golden 63 064 (AndDocIdSet / OrDocIdIterator / SVScanDocIdIterator) and, call by call, by
 * the reference's NotDocIdIteratorTest.java:31-104, AndDocIdIteratorTest.java:32-55 and OrDocIdIteratorTest.java:32-57 scripts (tests/test_oracle_iterator_scripts.py through po_not_iterator_script).
 *
 * The structure deliberately mirrors the JVM path so that timing it is a fair "port" CPU baseline:
 * 256-doc scan batches (BlockDocIdIterator.OPTIMAL_ITERATOR_BATCH_SIZE), 10 000-doc projection blocks
 * (DocIdSetPlanNode.MAX_DOC_PER_CALL), double result holders, one segment per thread.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pinot_gpu.h"

#define PO_SCAN_BATCH 256      /* core/common/BlockDocIdIterator.java:49 */
#define PO_MAX_DOC_PER_CALL 10000 /* core/plan/DocIdSetPlanNode.java:29 */
#define PO_MAX_GROUP_COLS 16   /* group-by key columns (the raw key is one 128-bit number: key spaces up to 2^96 x one more column) */
#define PO_EOF (-1)            /* segl Constants.EOF is Integer.MIN_VALUE in the reference; any negative works here */

static __thread char po_error[512];
const char* po_last_error(void) { return po_error; }
#define PO_FAIL(code, ...) do { snprintf(po_error, sizeof(po_error), __VA_ARGS__); return (code); } while (0)

/* ------------------------------------------------------------------------------------------------
 * PinotDataBuffer big-endian accessors (sspi/memory/PinotDataBuffer.java:375-444; files are BIG_ENDIAN,
 * segl/io/writer/impl/FixedBitSVForwardIndexWriter.java:43-44)
 * ---------------------------------------------------------------------------------------------- */
static inline int32_t be_get_int(const uint8_t* p) {
  return (int32_t)(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]);
}
static inline int64_t be_get_long(const uint8_t* p) {
  return (int64_t)(((uint64_t)(uint32_t)be_get_int(p) << 32) | (uint64_t)(uint32_t)be_get_int(p + 4));
}
static inline float be_get_float(const uint8_t* p) { int32_t i = be_get_int(p); float f; memcpy(&f, &i, 4); return f; }
static inline double be_get_double(const uint8_t* p) { int64_t i = be_get_long(p); double d; memcpy(&d, &i, 8); return d; }
static inline void be_put_int(uint8_t* p, int32_t v) {
  p[0] = (uint8_t)((uint32_t)v >> 24); p[1] = (uint8_t)((uint32_t)v >> 16); p[2] = (uint8_t)((uint32_t)v >> 8); p[3] = (uint8_t)v;
}

static inline void be_put_long(uint8_t* p, int64_t v) { be_put_int(p, (int32_t)((uint64_t)v >> 32)); be_put_int(p + 4, (int32_t)(uint64_t)v); }

/* ------------------------------------------------------------------------------------------------
 * PinotDataBitSet (segl/io/util/PinotDataBitSet.java)
 * ---------------------------------------------------------------------------------------------- */

/* getNumBitsPerValue, PinotDataBitSet.java:61-72 (FIRST_BIT_SET[v] = index from the MSB of the first set bit). */
int po_num_bits_per_value(int32_t max_value) {
  if (max_value <= 1) return 1;
  int num_bits = 8;
  uint32_t v = (uint32_t)max_value;
  while (v > 0xFF) { v >>= 8; num_bits += 8; }
  int first_bit_set = 0;
  while (!(v & (0x80u >> first_bit_set))) first_bit_set++;
  return num_bits - first_bit_set;
}

/* readInt(index, numBitsPerValue), PinotDataBitSet.java:80-104 -- byte-exact, never reads past the value. */
int32_t po_bitset_read_int(const uint8_t* buf, int64_t index, int num_bits) {
  int64_t bit_offset = index * num_bits;
  int64_t byte_offset = bit_offset / 8;
  int bit_offset_in_first_byte = (int)(bit_offset % 8);
  int32_t current = buf[byte_offset] & (0xFF >> bit_offset_in_first_byte);
  int num_bits_left = num_bits - (8 - bit_offset_in_first_byte);
  if (num_bits_left <= 0) {
    return (int32_t)((uint32_t)current >> -num_bits_left);
  }
  while (num_bits_left > 8) {
    byte_offset++;
    current = (int32_t)(((uint32_t)current << 8) | buf[byte_offset]);
    num_bits_left -= 8;
  }
  return (int32_t)(((uint32_t)current << num_bits_left) | ((uint32_t)buf[byte_offset + 1] >> (8 - num_bits_left)));
}

/* writeInt(index, numBitsPerValue, value), PinotDataBitSet.java:143-170 -- the layout authority. */
void po_bitset_write_int(uint8_t* buf, int64_t index, int num_bits, int32_t value) {
  int64_t bit_offset = index * num_bits;
  int64_t byte_offset = bit_offset / 8;
  int bit_offset_in_first_byte = (int)(bit_offset % 8);
  int first_byte = buf[byte_offset];
  int first_byte_mask = 0xFF >> bit_offset_in_first_byte;
  int num_bits_left = num_bits - (8 - bit_offset_in_first_byte);
  if (num_bits_left <= 0) {
    first_byte_mask &= 0xFF << -num_bits_left;
    buf[byte_offset] = (uint8_t)((first_byte & ~first_byte_mask) | ((uint32_t)value << -num_bits_left));
  } else {
    buf[byte_offset] = (uint8_t)((first_byte & ~first_byte_mask) | (((uint32_t)value >> num_bits_left) & first_byte_mask));
    while (num_bits_left > 8) {
      num_bits_left -= 8;
      byte_offset++;
      buf[byte_offset] = (uint8_t)(value >> num_bits_left);
    }
    byte_offset++;
    int last_byte = buf[byte_offset];
    buf[byte_offset] = (uint8_t)((last_byte & (0xFF >> num_bits_left)) | ((uint32_t)value << (8 - num_bits_left)));   /* Java's int shift wraps */
  }
}

/* FixedBitSVForwardIndexWriter (segl/io/writer/impl/FixedBitSVForwardIndexWriter.java:39-50): file length
 * ceil(numDocs * bits / 8), values written one by one through writeInt.  buf must be zero-initialised. */
int64_t po_fixedbit_file_size(int64_t num_docs, int num_bits) { return (num_docs * num_bits + 7) / 8; }
void po_fixedbit_write(uint8_t* buf, const int32_t* dict_ids, int64_t num_docs, int num_bits) {
  for (int64_t i = 0; i < num_docs; i++) po_bitset_write_int(buf, i, num_bits, dict_ids[i]);
}

/* ------------------------------------------------------------------------------------------------
 * FixedBitIntReader (segl/io/reader/impl/FixedBitIntReader.java): the reference hand-unrolls 31 classes;
 * all of them compute the closed form below (checked against Bit17Reader
 * :1268-1337).  read() is the bounded variant (byte-exact); readUnchecked() does one wide big-endian
 * load at floor(i*b/8) and may touch up to 7 bytes past the value; read32() decodes 32 values from b ints.
 * ---------------------------------------------------------------------------------------------- */
static inline int32_t fixedbit_read(const uint8_t* buf, int64_t index, int num_bits) {
  return po_bitset_read_int(buf, index, num_bits);
}
/* `size` = bytes of the file: the reference's readUnchecked may look up to 7 bytes past the value (harmless inside the JVM's
 * page-granular buffers: the extra bits are masked off); here a window that would leave the file is read byte-exactly instead,
 * which yields the same value. */
static inline int32_t fixedbit_read_unchecked(const uint8_t* buf, int64_t size, int64_t index, int num_bits) {
  int64_t bit_offset = index * num_bits;
  if ((bit_offset >> 3) + 8 > size) return po_bitset_read_int(buf, index, num_bits);
  const uint8_t* p = buf + (bit_offset >> 3);
  int bit_off = (int)(bit_offset & 7);
  uint32_t mask = (num_bits == 32) ? 0xFFFFFFFFu : ((1u << num_bits) - 1u);
  if (bit_off + num_bits <= 32) {
    /* e.g. Bit17Reader.readUnchecked :1278-1283: (getInt(off) >>> (15 - bitOff)) & 0x1ffff */
    return (int32_t)(((uint32_t)be_get_int(p) >> (32 - bit_off - num_bits)) & mask);
  }
  /* wider than an int window: the reference switches to getLong (e.g. Bit31Reader) */
  return (int32_t)(((uint64_t)be_get_long(p) >> (64 - bit_off - num_bits)) & mask);
}
static void fixedbit_read32(const uint8_t* buf, int64_t index, int num_bits, int32_t* out) {
  /* read32(index,...): offset = (index >>> 3) * b, loads b big-endian ints, emits 32 values
   * (FixedBitIntReader.java:1285-1337 for b = 17). */
  const uint8_t* p = buf + (index >> 3) * num_bits;
  uint32_t w[32];
  for (int j = 0; j < num_bits; j++) w[j] = (uint32_t)be_get_int(p + 4 * j);
  uint32_t mask = (1u << num_bits) - 1u;
  for (int k = 0; k < 32; k++) {
    int bit = k * num_bits;
    int j = bit >> 5, s = bit & 31;
    if (s + num_bits <= 32) {
      out[k] = (int32_t)((w[j] >> (32 - s - num_bits)) & mask);
    } else {
      int lo_bits = s + num_bits - 32;
      out[k] = (int32_t)(((w[j] << lo_bits) | (w[j + 1] >> (32 - lo_bits))) & mask);
    }
  }
}

/* FixedBitSVForwardIndexReaderV2.readDictIds (segl/segment/index/readers/forward/FixedBitSVForwardIndexReaderV2.java:65-99) */
void po_fixedbit_read_dict_ids(const uint8_t* buf, int num_bits, int32_t num_docs, const int32_t* doc_ids,
                               int32_t length, int32_t* dict_id_buffer) {
  if (length <= 0) return;
  const int64_t size = ((int64_t)num_docs * num_bits + 7) / 8;      /* FixedBitSVForwardIndexWriter.java:41-45: no header, no padding */
  int32_t first_doc_id = doc_ids[0];
  int32_t last_doc_id = doc_ids[length - 1];
  int32_t index = 0;
  /* Use bulk read if the doc ids are sequential */
  if (last_doc_id - first_doc_id + 1 == length && length >= 64) {
    int32_t bulk_start = (first_doc_id + 31) & (int32_t)0xffffffe0;
    int32_t bulk_end = last_doc_id & (int32_t)0xffffffe0;
    for (int32_t i = first_doc_id; i < bulk_start; i++) dict_id_buffer[index++] = fixedbit_read_unchecked(buf, size, i, num_bits);
    for (int32_t i = bulk_start; i < bulk_end; i += 32) {
      fixedbit_read32(buf, i, num_bits, dict_id_buffer + index);
      index += 32;
    }
  }
  /* Process the remaining docs */
  if (last_doc_id < num_docs - 2) {
    for (int32_t i = index; i < length; i++) dict_id_buffer[i] = fixedbit_read_unchecked(buf, size, doc_ids[i], num_bits);
  } else {
    dict_id_buffer[length - 1] = fixedbit_read(buf, last_doc_id, num_bits);
    int32_t unchecked_end = length - 2;
    if (unchecked_end >= index) {
      dict_id_buffer[unchecked_end] = fixedbit_read(buf, doc_ids[unchecked_end], num_bits);
      for (int32_t i = index; i < unchecked_end; i++) dict_id_buffer[i] = fixedbit_read_unchecked(buf, size, doc_ids[i], num_bits);
    }
  }
}

/* ------------------------------------------------------------------------------------------------
 * Raw fixed-byte chunk forward index, PASS_THROUGH (segl/segment/index/readers/forward/
 * BaseChunkForwardIndexReader.java:61-111, FixedByteChunkSVForwardIndexReader.java:53-61; writer
 * segl/io/writer/impl/BaseChunkForwardIndexWriter.java:130-163).
 * ---------------------------------------------------------------------------------------------- */
typedef struct po_raw_reader {
  int32_t version, num_chunks, num_docs_per_chunk, length_of_longest_entry, total_docs, compression_type;
  int32_t data_header_start, raw_data_start;
  const uint8_t* raw_data;
} po_raw_reader;

int po_raw_open(const uint8_t* buf, uint64_t size, po_raw_reader* r) {
  if (size < 16) PO_FAIL(1, "raw forward index too small");
  int off = 0;
  r->version = be_get_int(buf + off); off += 4;
  r->num_chunks = be_get_int(buf + off); off += 4;
  r->num_docs_per_chunk = be_get_int(buf + off); off += 4;
  r->length_of_longest_entry = be_get_int(buf + off); off += 4;
  int data_header_start = off;
  r->total_docs = -1;
  r->compression_type = 2; /* SNAPPY for version 1 */
  if (r->version > 1) {
    r->total_docs = be_get_int(buf + off); off += 4;
    r->compression_type = be_get_int(buf + off); off += 4;
    data_header_start = be_get_int(buf + off);
  }
  int entry = r->version <= 2 ? 4 : 8;
  r->data_header_start = data_header_start;
  r->raw_data_start = data_header_start + r->num_chunks * entry;
  r->raw_data = buf + r->raw_data_start;
  if (r->compression_type != 0) PO_FAIL(2, "only PASS_THROUGH raw chunks are in scope (compressionType=%d)", r->compression_type);
  return 0;
}
static inline int32_t raw_get_int(const po_raw_reader* r, int32_t doc_id) { return be_get_int(r->raw_data + (int64_t)doc_id * 4); }
/* FixedByteChunkSVForwardIndexReader.getLong/getFloat/getDouble :63-93: same addressing with the entry size of the type */
static inline int64_t raw_get_long(const po_raw_reader* r, int32_t doc_id) { return be_get_long(r->raw_data + (int64_t)doc_id * 8); }
static inline float raw_get_float(const po_raw_reader* r, int32_t doc_id) { return be_get_float(r->raw_data + (int64_t)doc_id * 4); }
static inline double raw_get_double(const po_raw_reader* r, int32_t doc_id) { return be_get_double(r->raw_data + (int64_t)doc_id * 8); }
/* header fields for tests (the reference's own fixedByteRaw.v2 fixture pins them) */
int po_raw_header(const uint8_t* buf, uint64_t size, int32_t* out8) {
  po_raw_reader r;
  if (po_raw_open(buf, size, &r)) return 1;
  out8[0] = r.version; out8[1] = r.num_chunks; out8[2] = r.num_docs_per_chunk; out8[3] = r.length_of_longest_entry;
  out8[4] = r.total_docs; out8[5] = r.compression_type; out8[6] = r.data_header_start; out8[7] = r.raw_data_start;
  return 0;
}

/* Writer restatement: version 2 header, 4-byte chunk offsets, PASS_THROUGH (value 0). Returns total size. */
int64_t po_raw_file_size_v2(int32_t num_docs, int32_t num_docs_per_chunk) {
  int64_t num_chunks = ((int64_t)num_docs + num_docs_per_chunk - 1) / num_docs_per_chunk;
  return 7 * 4 + num_chunks * 4 + (int64_t)num_docs * 4;
}
void po_raw_write_int_v2(uint8_t* buf, const int32_t* values, int32_t num_docs, int32_t num_docs_per_chunk) {
  int32_t num_chunks = (int32_t)(((int64_t)num_docs + num_docs_per_chunk - 1) / num_docs_per_chunk);
  int32_t header_size = 7 * 4 + num_chunks * 4;
  be_put_int(buf + 0, 2);
  be_put_int(buf + 4, num_chunks);
  be_put_int(buf + 8, num_docs_per_chunk);
  be_put_int(buf + 12, 4);
  be_put_int(buf + 16, num_docs);
  be_put_int(buf + 20, 0);   /* PASS_THROUGH */
  be_put_int(buf + 24, 28);  /* dataHeaderStart */
  for (int32_t c = 0; c < num_chunks; c++) be_put_int(buf + 28 + 4 * c, header_size + c * num_docs_per_chunk * 4);
  for (int32_t i = 0; i < num_docs; i++) be_put_int(buf + header_size + (int64_t)i * 4, values[i]);
}

/* Same writer for any fixed-width type: `values` is a host-order array of `entry_size`-byte elements (4 or 8). */
int64_t po_raw_file_size_typed_v2(int32_t num_docs, int32_t num_docs_per_chunk, int32_t entry_size) {
  int64_t num_chunks = ((int64_t)num_docs + num_docs_per_chunk - 1) / num_docs_per_chunk;
  return 7 * 4 + num_chunks * 4 + (int64_t)num_docs * entry_size;
}
void po_raw_write_typed_v2(uint8_t* buf, const void* values, int32_t num_docs, int32_t num_docs_per_chunk, int32_t entry_size) {
  int32_t num_chunks = (int32_t)(((int64_t)num_docs + num_docs_per_chunk - 1) / num_docs_per_chunk);
  int32_t header_size = 7 * 4 + num_chunks * 4;
  be_put_int(buf + 0, 2);
  be_put_int(buf + 4, num_chunks);
  be_put_int(buf + 8, num_docs_per_chunk);
  be_put_int(buf + 12, entry_size);
  be_put_int(buf + 16, num_docs);
  be_put_int(buf + 20, 0);
  be_put_int(buf + 24, 28);
  for (int32_t c = 0; c < num_chunks; c++) be_put_int(buf + 28 + 4 * c, header_size + c * num_docs_per_chunk * entry_size);
  for (int32_t i = 0; i < num_docs; i++) {
    if (entry_size == 4) { int32_t v; memcpy(&v, (const uint8_t*)values + (int64_t)i * 4, 4); be_put_int(buf + header_size + (int64_t)i * 4, v); }
    else { int64_t v; memcpy(&v, (const uint8_t*)values + (int64_t)i * 8, 8); be_put_long(buf + header_size + (int64_t)i * 8, v); }
  }
}

/* ------------------------------------------------------------------------------------------------
 * IntDictionary / BaseImmutableDictionary (segl/segment/index/readers/IntDictionary.java:38-70,
 * BaseImmutableDictionary.java:124-140; value access FixedByteValueReaderWriter.java:37-38)
 * ---------------------------------------------------------------------------------------------- */
static inline int32_t dict_get_int(const uint8_t* dict, int32_t dict_id) { return be_get_int(dict + (int64_t)dict_id * 4); }
int32_t po_dict_get_int(const uint8_t* dict, int32_t dict_id) { return dict_get_int(dict, dict_id); }

/* binarySearch(int value): returns index, or -(insertionPoint + 1) when absent. */
int32_t po_dict_insertion_index_of_int(const uint8_t* dict, int32_t length, int32_t value) {
  int32_t low = 0, high = length - 1;
  while (low <= high) {
    int32_t mid = (int32_t)(((uint32_t)low + (uint32_t)high) >> 1);
    int32_t mid_value = dict_get_int(dict, mid);
    if (mid_value < value) low = mid + 1;
    else if (mid_value > value) high = mid - 1;
    else return mid;
  }
  return -(low + 1);
}
/* indexOf -> normalizeIndex, BaseImmutableDictionary.java:73-80 */
int32_t po_dict_index_of_int(const uint8_t* dict, int32_t length, int32_t value) {
  int32_t idx = po_dict_insertion_index_of_int(dict, length, value);
  return idx >= 0 ? idx : -1;
}
void po_dict_write_int(uint8_t* buf, const int32_t* sorted_values, int32_t length) {
  /* SegmentDictionaryCreator.java:109-125: C x big-endian int32, ascending, no header */
  for (int32_t i = 0; i < length; i++) be_put_int(buf + (int64_t)i * 4, sorted_values[i]);
}

/* LongDictionary / FloatDictionary / DoubleDictionary (segl/segment/index/readers/{Long,Float,Double}Dictionary.java;
 * BaseImmutableDictionary.binarySearch(long|float|double) :142-195; FixedByteValueReaderWriter.getLong/getFloat/getDouble
 * :42-54): C x big-endian fixed-width values, ascending.  `value` arrives as the Java-parsed number widened to double for
 * FLOAT (Float.parseFloat) / DOUBLE and as int64 for LONG. */
static inline int64_t dict_get_long(const uint8_t* dict, int32_t dict_id) { return be_get_long(dict + (int64_t)dict_id * 8); }
static inline float dict_get_float(const uint8_t* dict, int32_t dict_id) { return be_get_float(dict + (int64_t)dict_id * 4); }
static inline double dict_get_double(const uint8_t* dict, int32_t dict_id) { return be_get_double(dict + (int64_t)dict_id * 8); }
#define PO_BSEARCH(NAME, T, GET)                                                                 \
  int32_t NAME(const uint8_t* dict, int32_t length, T value) {                                    \
    int32_t low = 0, high = length - 1;                                                           \
    while (low <= high) {                                                                         \
      int32_t mid = (int32_t)(((uint32_t)low + (uint32_t)high) >> 1);                              \
      T mid_value = GET(dict, mid);                                                               \
      if (mid_value < value) low = mid + 1;                                                       \
      else if (mid_value > value) high = mid - 1;                                                 \
      else return mid;                                                                            \
    }                                                                                             \
    return -(low + 1);                                                                            \
  }
PO_BSEARCH(po_dict_insertion_index_of_long, int64_t, dict_get_long)
PO_BSEARCH(po_dict_insertion_index_of_float, float, dict_get_float)
PO_BSEARCH(po_dict_insertion_index_of_double, double, dict_get_double)
void po_dict_write_long(uint8_t* buf, const int64_t* sorted_values, int32_t length) {
  for (int32_t i = 0; i < length; i++) be_put_long(buf + (int64_t)i * 8, sorted_values[i]);
}
void po_dict_write_float(uint8_t* buf, const float* sorted_values, int32_t length) {
  for (int32_t i = 0; i < length; i++) { int32_t b; memcpy(&b, &sorted_values[i], 4); be_put_int(buf + (int64_t)i * 4, b); }
}
void po_dict_write_double(uint8_t* buf, const double* sorted_values, int32_t length) {
  for (int32_t i = 0; i < length; i++) { int64_t b; memcpy(&b, &sorted_values[i], 8); be_put_long(buf + (int64_t)i * 8, b); }
}
/* insertionIndexOf for any stored type; the bound is given as int64 (INT / LONG) or double (FLOAT / DOUBLE) */
int32_t po_dict_insertion_index_of(const uint8_t* dict, int32_t length, int stored_type, int64_t ivalue, double dvalue) {
  switch (stored_type) {
    case PG_TYPE_INT: return po_dict_insertion_index_of_int(dict, length, (int32_t)ivalue);
    case PG_TYPE_LONG: return po_dict_insertion_index_of_long(dict, length, ivalue);
    case PG_TYPE_FLOAT: return po_dict_insertion_index_of_float(dict, length, (float)dvalue);
    default: return po_dict_insertion_index_of_double(dict, length, dvalue);
  }
}
/* the same bound rules as po_lower_range_int for any stored type */
void po_lower_range_typed(const uint8_t* dict, int32_t length, int stored_type, int has_lower, int64_t ilower, double dlower, int lower_inclusive,
                          int has_upper, int64_t iupper, double dupper, int upper_inclusive, int32_t* out_start, int32_t* out_end) {
  int32_t start, end;
  if (!has_lower) start = 0;
  else {
    int32_t ins = po_dict_insertion_index_of(dict, length, stored_type, ilower, dlower);
    start = ins < 0 ? -(ins + 1) : (lower_inclusive ? ins : ins + 1);
  }
  if (!has_upper) end = length;
  else {
    int32_t ins = po_dict_insertion_index_of(dict, length, stored_type, iupper, dupper);
    end = ins < 0 ? -(ins + 1) : (upper_inclusive ? ins + 1 : ins);
  }
  *out_start = start;
  *out_end = end;
}

/* SortedDictionaryBasedRangePredicateEvaluator ctor (core/operator/filter/predicate/
 * RangePredicateEvaluatorFactory.java:126-169): bounds -> [startDictId, endDictId). */
void po_lower_range_int(const uint8_t* dict, int32_t length, int has_lower, int32_t lower, int lower_inclusive,
                        int has_upper, int32_t upper, int upper_inclusive, int32_t* out_start, int32_t* out_end) {
  int32_t start, end;
  if (!has_lower) {
    start = 0;
  } else {
    int32_t ins = po_dict_insertion_index_of_int(dict, length, lower);
    if (ins < 0) start = -(ins + 1);
    else start = lower_inclusive ? ins : ins + 1;
  }
  if (!has_upper) {
    end = length;
  } else {
    int32_t ins = po_dict_insertion_index_of_int(dict, length, upper);
    if (ins < 0) end = -(ins + 1);
    else end = upper_inclusive ? ins + 1 : ins;
  }
  *out_start = start;
  *out_end = end;
}

/* ------------------------------------------------------------------------------------------------
 * RoaringBitmap portable serialization (third-party; public RoaringFormatSpec).  Call sites in the
 * reference: BitmapInvertedIndexReader.java:57 (deserialize view), BitmapInvertedIndexWriter.java:90-96.
 * ---------------------------------------------------------------------------------------------- */
static inline uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
static inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static inline void put_le16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
static inline void put_le32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

#define ROARING_COOKIE_NO_RUN 12346u
#define ROARING_COOKIE_RUN 12347u
#define ROARING_NO_OFFSET_THRESHOLD 4

/* ORs the serialized bitmap into a dense bitmap (bit d&63 of words[d>>6]); returns cardinality or -1. */
int64_t po_roaring_or_into(const uint8_t* data, uint64_t size, uint64_t* words, int64_t num_words) {
  if (size < 8) { snprintf(po_error, sizeof(po_error), "roaring: truncated"); return -1; }
  uint32_t cookie = le32(data);
  uint32_t n;
  const uint8_t* run_flags = NULL;
  uint64_t pos;
  int has_run = 0;
  if ((cookie & 0xFFFF) == ROARING_COOKIE_RUN) {
    has_run = 1;
    n = (cookie >> 16) + 1;
    run_flags = data + 4;
    pos = 4 + (n + 7) / 8;
  } else if (cookie == ROARING_COOKIE_NO_RUN) {
    n = le32(data + 4);
    pos = 8;
  } else { snprintf(po_error, sizeof(po_error), "roaring: bad cookie %u", cookie); return -1; }
  const uint8_t* desc = data + pos;
  pos += (uint64_t)n * 4;
  if (!has_run || n >= ROARING_NO_OFFSET_THRESHOLD) pos += (uint64_t)n * 4; /* offset header (not needed: containers are sequential) */
  int64_t total = 0;
  for (uint32_t c = 0; c < n; c++) {
    uint32_t key = le16(desc + 4 * c);
    uint32_t card = (uint32_t)le16(desc + 4 * c + 2) + 1;
    int64_t base_word = (int64_t)key * 1024;
    int is_run = has_run && ((run_flags[c >> 3] >> (c & 7)) & 1);
    if (is_run) {
      uint32_t num_runs = le16(data + pos); pos += 2;
      for (uint32_t r = 0; r < num_runs; r++) {
        uint32_t start = le16(data + pos), len = le16(data + pos + 2); pos += 4;
        for (uint32_t v = start; v <= start + len; v++) {
          int64_t w = base_word + (v >> 6);
          if (w >= num_words) { snprintf(po_error, sizeof(po_error), "roaring: value out of range"); return -1; }
          words[w] |= 1ull << (v & 63);
        }
      }
    } else if (card > 4096) {
      for (int j = 0; j < 1024; j++) {
        uint64_t v = (uint64_t)le32(data + pos) | ((uint64_t)le32(data + pos + 4) << 32); pos += 8;
        if (v) {
          if (base_word + j >= num_words) { snprintf(po_error, sizeof(po_error), "roaring: value out of range"); return -1; }
          words[base_word + j] |= v;
        }
      }
    } else {
      for (uint32_t i = 0; i < card; i++) {
        uint32_t v = le16(data + pos); pos += 2;
        int64_t w = base_word + (v >> 6);
        if (w >= num_words) { snprintf(po_error, sizeof(po_error), "roaring: value out of range"); return -1; }
        words[w] |= 1ull << (v & 63);
      }
    }
    total += card;
    if (pos > size) { snprintf(po_error, sizeof(po_error), "roaring: truncated container"); return -1; }
  }
  return total;
}

/* Serializer used to build synthetic postings: sorted distinct docIds -> portable format.  Container choice
 * follows the library: array when card <= 4096 else bitset, then runOptimize() (what
 * RoaringBitmapWriter.writer().get() does on flush; OffHeapBitmapInvertedIndexCreator.java:235-249):
 * convert to a run container when its serialized size 2 + 4*numRuns is smaller.
 * Returns the size; writes when out != NULL. */
int64_t po_roaring_serialize(const int32_t* doc_ids, int64_t n, int run_optimize, uint8_t* out) {
  /* pass 1: container boundaries */
  int64_t num_containers = 0;
  for (int64_t i = 0; i < n;) {
    uint32_t key = (uint32_t)doc_ids[i] >> 16;
    while (i < n && ((uint32_t)doc_ids[i] >> 16) == key) i++;
    num_containers++;
  }
  uint32_t* keys = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(num_containers + 1));
  int64_t* starts = (int64_t*)malloc(sizeof(int64_t) * (size_t)(num_containers + 1));
  uint8_t* kinds = (uint8_t*)malloc((size_t)num_containers + 1); /* 0 array, 1 bitset, 2 run */
  uint32_t* num_runs = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(num_containers + 1));
  int64_t c = 0;
  int any_run = 0;
  for (int64_t i = 0; i < n;) {
    uint32_t key = (uint32_t)doc_ids[i] >> 16;
    keys[c] = key; starts[c] = i;
    uint32_t runs = 0; int64_t j = i;
    while (j < n && ((uint32_t)doc_ids[j] >> 16) == key) {
      if (j == i || doc_ids[j] != doc_ids[j - 1] + 1) runs++;
      j++;
    }
    int64_t card = j - i;
    int64_t plain_size = card > 4096 ? 8192 : 2 * card;
    kinds[c] = card > 4096 ? 1 : 0;
    num_runs[c] = runs;
    if (run_optimize && 2 + 4 * (int64_t)runs < plain_size) { kinds[c] = 2; any_run = 1; }
    i = j; c++;
  }
  starts[num_containers] = n;
  /* header */
  int64_t pos = 0;
  if (any_run) {
    if (out) { put_le32(out, ROARING_COOKIE_RUN | ((uint32_t)(num_containers - 1) << 16)); memset(out + 4, 0, (size_t)((num_containers + 7) / 8)); }
    pos = 4 + (num_containers + 7) / 8;
    if (out) for (int64_t k = 0; k < num_containers; k++) if (kinds[k] == 2) out[4 + (k >> 3)] |= (uint8_t)(1u << (k & 7));
  } else {
    if (out) { put_le32(out, ROARING_COOKIE_NO_RUN); put_le32(out + 4, (uint32_t)num_containers); }
    pos = 8;
  }
  for (int64_t k = 0; k < num_containers; k++) {
    if (out) { put_le16(out + pos, keys[k]); put_le16(out + pos + 2, (uint32_t)(starts[k + 1] - starts[k] - 1)); }
    pos += 4;
  }
  int64_t offset_header_pos = -1;
  if (!any_run || num_containers >= ROARING_NO_OFFSET_THRESHOLD) { offset_header_pos = pos; pos += 4 * num_containers; }
  for (int64_t k = 0; k < num_containers; k++) {
    if (offset_header_pos >= 0 && out) put_le32(out + offset_header_pos + 4 * k, (uint32_t)pos);
    int64_t s = starts[k], e = starts[k + 1];
    if (kinds[k] == 0) {
      if (out) for (int64_t i = s; i < e; i++) put_le16(out + pos + 2 * (i - s), (uint32_t)doc_ids[i] & 0xFFFF);
      pos += 2 * (e - s);
    } else if (kinds[k] == 1) {
      if (out) {
        memset(out + pos, 0, 8192);
        for (int64_t i = s; i < e; i++) { uint32_t v = (uint32_t)doc_ids[i] & 0xFFFF; out[pos + (v >> 3)] |= (uint8_t)(1u << (v & 7)); }
      }
      pos += 8192;
    } else {
      if (out) put_le16(out + pos, num_runs[k]);
      pos += 2;
      int64_t i = s;
      while (i < e) {
        int64_t j = i;
        while (j + 1 < e && doc_ids[j + 1] == doc_ids[j] + 1) j++;
        if (out) { put_le16(out + pos, (uint32_t)doc_ids[i] & 0xFFFF); put_le16(out + pos + 2, (uint32_t)(j - i)); }
        pos += 4;
        i = j + 1;
      }
    }
  }
  free(keys); free(starts); free(kinds); free(num_runs);
  return pos;
}

/* BitmapInvertedIndexReader (segl/segment/index/readers/BitmapInvertedIndexReader.java:45-62):
 * (numBitmaps + 1) big-endian uint32 offsets, then the serialized bitmaps; offsets are relative to the
 * first offset (the reader subtracts _firstOffset). */
int po_inverted_get(const uint8_t* inv, uint64_t inv_size, int32_t num_bitmaps, int32_t dict_id,
                    const uint8_t** out_data, uint64_t* out_len) {
  if (dict_id < 0 || dict_id >= num_bitmaps) PO_FAIL(1, "inverted index: dictId %d out of range", dict_id);
  uint64_t offset_buffer_end = ((uint64_t)num_bitmaps + 1) * 4;
  uint64_t first_offset = (uint32_t)be_get_int(inv);
  uint64_t offset = (uint32_t)be_get_int(inv + (uint64_t)dict_id * 4);
  uint64_t length = (uint32_t)be_get_int(inv + ((uint64_t)dict_id + 1) * 4) - offset;
  *out_data = inv + offset_buffer_end + (offset - first_offset);
  *out_len = length;
  if (offset_buffer_end + (offset - first_offset) + length > inv_size) PO_FAIL(1, "inverted index: bitmap past end of buffer");
  return 0;
}

/* BitmapInvertedIndexWriter layout (segl/segment/creator/impl/inv/BitmapInvertedIndexWriter.java:35-50,90-97):
 * offsets are absolute positions in the file (first offset = (numBitmaps + 1) * 4). */
int64_t po_inverted_build(const int32_t* dict_ids, int32_t num_docs, int32_t cardinality, int run_optimize, uint8_t* out) {
  /* counting sort of docIds by dictId (postings are ascending docIds) */
  int64_t* starts = (int64_t*)calloc((size_t)cardinality + 1, sizeof(int64_t));
  for (int32_t i = 0; i < num_docs; i++) starts[dict_ids[i] + 1]++;
  for (int32_t d = 0; d < cardinality; d++) starts[d + 1] += starts[d];
  int32_t* postings = (int32_t*)malloc(sizeof(int32_t) * (size_t)(num_docs > 0 ? num_docs : 1));
  int64_t* fill = (int64_t*)malloc(sizeof(int64_t) * (size_t)(cardinality + 1));
  memcpy(fill, starts, sizeof(int64_t) * (size_t)(cardinality + 1));
  for (int32_t i = 0; i < num_docs; i++) postings[fill[dict_ids[i]]++] = i;
  int64_t pos = ((int64_t)cardinality + 1) * 4;
  for (int32_t d = 0; d < cardinality; d++) {
    if (out) be_put_int(out + (int64_t)d * 4, (int32_t)(uint32_t)pos);
    pos += po_roaring_serialize(postings + starts[d], starts[d + 1] - starts[d], run_optimize, out ? out + pos : NULL);
  }
  if (out) be_put_int(out + (int64_t)cardinality * 4, (int32_t)(uint32_t)pos);
  free(starts); free(postings); free(fill);
  return pos;
}

/* ------------------------------------------------------------------------------------------------
 * Query execution: FilterPlanNode -> DocIdSetOperator -> ProjectionOperator -> AggregationOperator /
 * GroupByOperator, one thread, pull model.
 * ---------------------------------------------------------------------------------------------- */
typedef struct po_column {
  const pg_column_desc* desc;
  po_raw_reader raw;           /* valid for RAW_FIXED_BYTE */
} po_column;

/* PredicateEvaluator.applySV on one dictId / raw value (RangePredicateEvaluatorFactory.java:220-222,
 * 364-366; EqualsPredicateEvaluatorFactory.java:122-124; InPredicateEvaluatorFactory.java:186-188;
 * NOT_EQ / NOT_IN evaluators are the negations). */
static inline int pred_apply(const pg_predicate* p, int64_t v) {
  int m;
  switch (p->kind) {
    case PG_PRED_MATCH_ALL: m = 1; break;
    case PG_PRED_MATCH_NONE: m = 0; break;
    case PG_PRED_DICT_RANGE: m = (p->lo <= v && p->hi > v); break;
    case PG_PRED_DICT_SET: m = (v >= 0 && (v >> 5) < p->num_set_words) ? (int)((p->set_words[v >> 5] >> (v & 31)) & 1u) : 0; break;
    case PG_PRED_RAW_RANGE: m = (v >= p->lo && v <= p->hi); break;
    default: m = 0;
  }
  return p->exclusive ? !m : m;
}

/* PG_PRED_RAW_SET: Int / Long / Float / DoubleRawValueBasedInPredicateEvaluator.applySV (InPredicateEvaluatorFactory.java:215-300):
 * _matchingValues.contains(value) on the column's own type.  On the ABI (include/pinot_gpu.h) the list travels as 64-bit patterns, two
 * set words per value, low word first: the long for INT / LONG columns (an int widened), the bits of the double for FLOAT / DOUBLE
 * columns (a float widened exactly) -- so one 64-bit compare restates all four evaluators: a long outside int32 never equals a widened
 * int, a double that is not a float never equals a widened float.  The fastutil float / double sets compare floatToIntBits /
 * doubleToLongBits; for everything but the zeros and NaN that is ==, and lists holding those are not offloaded (they never get here
 * from the tests that compare with the device).  Any order, duplicates allowed; an empty list matches nothing. */
static inline int raw_set_contains(const pg_predicate* p, uint64_t bits) {
  const int32_t nv = p->num_set_words / PG_RAW_SET_WORDS_PER_VALUE;
  for (int32_t i = 0; i < nv; i++) {
    if (((uint64_t)p->set_words[2 * i] | ((uint64_t)p->set_words[2 * i + 1] << 32)) == bits) return 1;
  }
  return 0;
}

/* SVScanDocIdIterator (core/operator/dociditerators/SVScanDocIdIterator.java:76-98, 213-243):
 * fills 256 sequential docIds, reads their dictIds / values, compacts the matches in place. */
typedef struct po_scan_iter {
  const po_column* col;
  const pg_predicate* pred;
  int32_t num_docs;
  int32_t next_doc_id;
  int32_t batch[PO_SCAN_BATCH];
  int32_t buffer[PO_SCAN_BATCH];
  int32_t first_mismatch, cursor;
  int64_t num_entries_scanned;
} po_scan_iter;

static void scan_iter_init(po_scan_iter* it, const po_column* col, const pg_predicate* pred, int32_t num_docs) {
  memset(it, 0, sizeof(*it));
  it->col = col; it->pred = pred; it->num_docs = num_docs;
}

/* ValueMatcher.matchValues: readDictIds / readValuesSV then predicateEvaluator.applySV(limit, docIds, values) */
static int32_t scan_match_values(po_scan_iter* it, int32_t limit, int32_t* doc_ids) {
  const pg_column_desc* d = it->col->desc;
  if (d->fwd_encoding == PG_FWD_FIXED_BIT_DICT) {
    po_fixedbit_read_dict_ids((const uint8_t*)d->fwd_data, d->bits_per_value, it->num_docs, doc_ids, limit, it->buffer);
  } else if (it->pred->kind == PG_PRED_RAW_SET) {
    int32_t matches = 0;
    for (int32_t i = 0; i < limit; i++) {
      uint64_t bits;
      if (d->stored_type == PG_TYPE_INT) bits = (uint64_t)(int64_t)raw_get_int(&it->col->raw, doc_ids[i]);
      else if (d->stored_type == PG_TYPE_LONG) bits = (uint64_t)raw_get_long(&it->col->raw, doc_ids[i]);
      else {
        const double v = d->stored_type == PG_TYPE_FLOAT ? (double)raw_get_float(&it->col->raw, doc_ids[i]) : raw_get_double(&it->col->raw, doc_ids[i]);
        memcpy(&bits, &v, 8);
      }
      const int m = raw_set_contains(it->pred, bits);
      if (it->pred->exclusive ? !m : m) doc_ids[matches++] = doc_ids[i];
    }
    return matches;
  } else if (d->stored_type == PG_TYPE_FLOAT || d->stored_type == PG_TYPE_DOUBLE) {
    /* Float / DoubleRawValueBasedRangePredicateEvaluator.applySV, RangePredicateEvaluatorFactory.java:448-560:
     * value >= inclusiveLowerBound && value <= inclusiveUpperBound on primitives (NaN never matches, -0.0 == 0.0) */
    double lo, hi;
    memcpy(&lo, &it->pred->lo, 8); memcpy(&hi, &it->pred->hi, 8);
    int32_t matches = 0;
    for (int32_t i = 0; i < limit; i++) {
      double v = d->stored_type == PG_TYPE_FLOAT ? (double)raw_get_float(&it->col->raw, doc_ids[i]) : raw_get_double(&it->col->raw, doc_ids[i]);
      int m = (it->pred->kind == PG_PRED_RAW_RANGE) ? (v >= lo && v <= hi) : (it->pred->kind == PG_PRED_MATCH_ALL);
      if (it->pred->exclusive ? !m : m) doc_ids[matches++] = doc_ids[i];
    }
    return matches;
  } else if (d->stored_type == PG_TYPE_LONG) {
    /* LongRawValueBasedRangePredicateEvaluator.applySV(long), RangePredicateEvaluatorFactory.java:411-446 */
    int32_t matches = 0;
    for (int32_t i = 0; i < limit; i++) {
      if (pred_apply(it->pred, raw_get_long(&it->col->raw, doc_ids[i]))) doc_ids[matches++] = doc_ids[i];
    }
    return matches;
  } else {
    for (int32_t i = 0; i < limit; i++) it->buffer[i] = raw_get_int(&it->col->raw, doc_ids[i]);
  }
  int32_t matches = 0;
  for (int32_t i = 0; i < limit; i++) {
    if (pred_apply(it->pred, it->buffer[i])) doc_ids[matches++] = doc_ids[i];
  }
  return matches;
}

static int32_t scan_iter_next(po_scan_iter* it) {
  if (it->cursor >= it->first_mismatch) {
    int32_t limit, batch_size = 0;
    do {
      limit = it->num_docs - it->next_doc_id;
      if (limit > PO_SCAN_BATCH) limit = PO_SCAN_BATCH;
      if (limit > 0) {
        for (int32_t i = 0; i < limit; i++) it->batch[i] = it->next_doc_id + i;
        batch_size = scan_match_values(it, limit, it->batch);
        it->next_doc_id += limit;
        it->num_entries_scanned += limit;
      }
    } while ((limit > 0) & (batch_size == 0));
    it->first_mismatch = batch_size;
    it->cursor = 0;
    if (it->first_mismatch == 0) return PO_EOF;
  }
  return it->batch[it->cursor++];
}

/* Dense docId bitmap helpers (stand in for MutableRoaringBitmap: same set semantics). */
static inline int64_t bitmap_words(int32_t num_docs) { return ((int64_t)num_docs + 63) / 64; }
static void bitmap_clear_tail(uint64_t* w, int32_t num_docs) {
  int r = num_docs & 63;
  if (r) w[num_docs >> 6] &= (1ull << r) - 1ull;
}

/* Evaluate one leaf into a dense bitmap.
 *  - scan leaf: the full-column scan of SVScanDocIdIterator.next() (256-doc batches)
 *  - inverted leaf: InvertedIndexFilterOperator.getTrues (core/operator/filter/InvertedIndexFilterOperator.java:60-96):
 *    OR of the postings of the matching dictIds; exclusive predicates flip over [0, numDocs). */
static int leaf_to_bitmap(const po_column* cols, const pg_segment_desc* seg, const pg_predicate* p, uint64_t* words,
                          int64_t* entries_scanned) {
  int32_t num_docs = seg->num_docs;
  int64_t nw = bitmap_words(num_docs);
  memset(words, 0, (size_t)nw * 8);
  if (p->kind == PG_PRED_MATCH_ALL || p->kind == PG_PRED_MATCH_NONE) {
    int all = (p->kind == PG_PRED_MATCH_ALL) != (p->exclusive != 0);
    if (all) { memset(words, 0xFF, (size_t)nw * 8); bitmap_clear_tail(words, num_docs); }
    return 0;
  }
  if (p->kind == PG_PRED_IS_NULL) {
    /* FilterPlanNode.java:294-310: BitmapBasedFilterOperator(nullBitmap, exclusive = IS_NOT_NULL); no null vector -> EmptyFilterOperator
     * (IS_NULL) / MatchAllFilterOperator (IS_NOT_NULL).  BitmapBasedFilterOperator.getTrues :41-47 flips over [0, numDocs). */
    if (p->column < 0 || p->column >= seg->num_columns) PO_FAIL(1, "IS_NULL column out of range");
    const pg_column_desc* d = &seg->columns[p->column];
    if (d->null_data && d->null_size) { if (po_roaring_or_into((const uint8_t*)d->null_data, d->null_size, words, nw) < 0) return 1; bitmap_clear_tail(words, num_docs); }
    if (p->exclusive) { for (int64_t i = 0; i < nw; i++) words[i] = ~words[i]; bitmap_clear_tail(words, num_docs); }
    return 0;
  }
  if (p->kind == PG_PRED_DOC_RANGE) {
    /* SortedIndexBasedFilterOperator.getTrues -> SortedDocIdSet of one inclusive [start, end] pair (:60-85); exclusive
     * predicates take the complement over [0, numDocs) (:72-84).  No entries are scanned. */
    int64_t lo = p->lo < 0 ? 0 : p->lo, hi = p->hi >= num_docs ? (int64_t)num_docs - 1 : p->hi;
    for (int64_t d = lo; d <= hi; d++) words[d >> 6] |= 1ull << (d & 63);
    if (p->exclusive) { for (int64_t i = 0; i < nw; i++) words[i] = ~words[i]; bitmap_clear_tail(words, num_docs); }
    return 0;
  }
  const po_column* col = &cols[p->column];
  if (p->eval == PG_EVAL_INVERTED) {
    const pg_column_desc* d = col->desc;
    if (!d->inv_data) PO_FAIL(1, "column %s has no inverted index", d->name);
    for (int32_t dict_id = 0; dict_id < d->cardinality; dict_id++) {
      pg_predicate inner = *p; inner.exclusive = 0;
      if (!pred_apply(&inner, dict_id)) continue;
      const uint8_t* data; uint64_t len;
      if (po_inverted_get((const uint8_t*)d->inv_data, d->inv_size, d->cardinality, dict_id, &data, &len)) return 1;
      if (po_roaring_or_into(data, len, words, nw) < 0) return 1;
    }
    if (p->exclusive) { for (int64_t i = 0; i < nw; i++) words[i] = ~words[i]; bitmap_clear_tail(words, num_docs); }
    return 0;
  }
  po_scan_iter it;
  scan_iter_init(&it, col, p, num_docs);
  int32_t doc;
  while ((doc = scan_iter_next(&it)) != PO_EOF) words[doc >> 6] |= 1ull << (doc & 63);
  *entries_scanned += it.num_entries_scanned;
  return 0;
}

/* The null bitmap of a column as dense words, or NULL when the column has no null docs (NullValueVectorReaderImpl.getNullBitmap). */
static uint64_t* column_null_words(const pg_segment_desc* seg, int32_t column) {
  if (column < 0 || column >= seg->num_columns) return NULL;
  const pg_column_desc* d = &seg->columns[column];
  if (!d->null_data || !d->null_size) return NULL;
  int64_t nw = bitmap_words(seg->num_docs);
  uint64_t* w = (uint64_t*)calloc((size_t)(nw ? nw : 1), 8);
  int64_t card = po_roaring_or_into((const uint8_t*)d->null_data, d->null_size, w, nw);
  bitmap_clear_tail(w, seg->num_docs);
  int64_t in_range = 0;
  for (int64_t i = 0; i < nw; i++) in_range += __builtin_popcountll(w[i]);
  if (card < 0 || in_range == 0) { free(w); return NULL; }   /* nullBitmap.isEmpty() */
  return w;
}

/* enableNullHandling=true: every filter operator has three docId sets (BaseFilterOperator.java:85-113):
 *   column leaf   trues = matches AND NOT nulls, nulls = the column's null bitmap (BaseColumnFilterOperator.java:45-64),
 *                 falses = NOT (trues OR nulls) (BaseFilterOperator.getFalses :96-113)
 *   IS_NULL / MATCH_ALL / MATCH_NONE leaves: no nulls, falses = NOT trues
 *   AND  trues = AND trues_i, falses = NOT AND_i (trues_i OR nulls_i) (AndFilterOperator.java:52-90); no nulls of its own
 *   OR   trues = OR trues_i,  falses = NOT OR_i (trues_i OR nulls_i)  (OrFilterOperator.java:51-89); no nulls of its own
 *   NOT  trues = child falses, falses = child trues (NotFilterOperator.java:52-63); no nulls of its own
 * The filter block is getTrues() of the root (BaseFilterOperator.getNextBlock :82-84). */
typedef struct po_tnf { uint64_t *t, *n, *f; } po_tnf;
static void tnf_free(po_tnf* e) { free(e->t); free(e->n); free(e->f); }
static int filter_to_bitmap_nulls(const po_column* cols, const pg_segment_desc* seg, const pg_query* q, uint64_t** out_words,
                                  int64_t* entries_scanned) {
  int32_t num_docs = seg->num_docs;
  int64_t nw = bitmap_words(num_docs);
  size_t bytes = (size_t)(nw ? nw : 1) * 8;
  po_tnf* stack = (po_tnf*)calloc((size_t)q->num_filter_nodes, sizeof(po_tnf));
  int sp = 0, rc = 0;
  for (int32_t n = 0; n < q->num_filter_nodes && !rc; n++) {
    const pg_filter_node* node = &q->filter[n];
    if (node->op == PG_FILTER_LEAF) {
      const pg_predicate* p = &q->predicates[node->predicate];
      po_tnf e; e.t = (uint64_t*)malloc(bytes); e.n = (uint64_t*)calloc(1, bytes); e.f = (uint64_t*)malloc(bytes);
      rc = leaf_to_bitmap(cols, seg, p, e.t, entries_scanned);
      const int column_leaf = p->kind == PG_PRED_DICT_RANGE || p->kind == PG_PRED_DICT_SET || p->kind == PG_PRED_RAW_RANGE || p->kind == PG_PRED_RAW_SET || p->kind == PG_PRED_DOC_RANGE;
      uint64_t* nulls = (!rc && column_leaf) ? column_null_words(seg, p->column) : NULL;
      if (nulls) { for (int64_t i = 0; i < nw; i++) { e.n[i] = nulls[i]; e.t[i] &= ~nulls[i]; } free(nulls); }
      for (int64_t i = 0; i < nw; i++) e.f[i] = ~(e.t[i] | e.n[i]);
      bitmap_clear_tail(e.f, num_docs);
      stack[sp++] = e;
    } else if (node->op == PG_FILTER_NOT) {
      if (sp < 1) { rc = 1; snprintf(po_error, sizeof(po_error), "filter stack underflow"); break; }
      po_tnf* e = &stack[sp - 1];
      uint64_t* t = e->t; e->t = e->f; e->f = t;
      memset(e->n, 0, bytes);
    } else {
      int k = node->num_children;
      if (sp < k || k < 1) { rc = 1; snprintf(po_error, sizeof(po_error), "filter stack underflow"); break; }
      po_tnf* acc = &stack[sp - k];
      /* acc.f is reused as the running AND / OR of (trues_i OR nulls_i) */
      for (int64_t i = 0; i < nw; i++) acc->f[i] = acc->t[i] | acc->n[i];
      for (int c = 1; c < k; c++) {
        po_tnf* w = &stack[sp - k + c];
        if (node->op == PG_FILTER_AND) for (int64_t i = 0; i < nw; i++) { acc->t[i] &= w->t[i]; acc->f[i] &= (w->t[i] | w->n[i]); }
        else for (int64_t i = 0; i < nw; i++) { acc->t[i] |= w->t[i]; acc->f[i] |= (w->t[i] | w->n[i]); }
        tnf_free(w);
      }
      for (int64_t i = 0; i < nw; i++) acc->f[i] = ~acc->f[i];
      bitmap_clear_tail(acc->f, num_docs);
      memset(acc->n, 0, bytes);
      sp -= k - 1;
    }
  }
  if (!rc && sp != 1) { rc = 1; snprintf(po_error, sizeof(po_error), "malformed filter tree"); }
  if (rc) { for (int i = 0; i < sp; i++) tnf_free(&stack[i]); free(stack); return 1; }
  *out_words = stack[0].t;
  free(stack[0].n); free(stack[0].f);
  free(stack);
  return 0;
}

/* AND / OR / NOT over docId sets (AndDocIdSet.java:110-172 intersects; OrDocIdSet unions; NotDocIdSet
 * complements over [0, numDocs)).  Postfix evaluation of the flattened tree. */
static int filter_to_bitmap(const po_column* cols, const pg_segment_desc* seg, const pg_query* q, uint64_t** out_words,
                            int64_t* entries_scanned) {
  int32_t num_docs = seg->num_docs;
  int64_t nw = bitmap_words(num_docs);
  if ((q->flags & PG_QUERY_NULL_HANDLING) && q->num_filter_nodes > 0) return filter_to_bitmap_nulls(cols, seg, q, out_words, entries_scanned);
  if (q->num_filter_nodes == 0) {
    uint64_t* w = (uint64_t*)malloc((size_t)(nw ? nw : 1) * 8);
    memset(w, 0xFF, (size_t)nw * 8); bitmap_clear_tail(w, num_docs);
    *out_words = w;
    return 0;
  }
  uint64_t** stack = (uint64_t**)calloc((size_t)q->num_filter_nodes, sizeof(uint64_t*));
  int sp = 0, rc = 0;
  for (int32_t n = 0; n < q->num_filter_nodes && !rc; n++) {
    const pg_filter_node* node = &q->filter[n];
    if (node->op == PG_FILTER_LEAF) {
      uint64_t* w = (uint64_t*)malloc((size_t)(nw ? nw : 1) * 8);
      rc = leaf_to_bitmap(cols, seg, &q->predicates[node->predicate], w, entries_scanned);
      stack[sp++] = w;
    } else if (node->op == PG_FILTER_NOT) {
      if (sp < 1) { rc = 1; snprintf(po_error, sizeof(po_error), "filter stack underflow"); break; }
      uint64_t* w = stack[sp - 1];
      for (int64_t i = 0; i < nw; i++) w[i] = ~w[i];
      bitmap_clear_tail(w, num_docs);
    } else {
      int k = node->num_children;
      if (sp < k || k < 1) { rc = 1; snprintf(po_error, sizeof(po_error), "filter stack underflow"); break; }
      uint64_t* acc = stack[sp - k];
      for (int c = 1; c < k; c++) {
        uint64_t* w = stack[sp - k + c];
        if (node->op == PG_FILTER_AND) for (int64_t i = 0; i < nw; i++) acc[i] &= w[i];
        else for (int64_t i = 0; i < nw; i++) acc[i] |= w[i];
        free(w);
      }
      sp -= k - 1;
    }
  }
  if (!rc && sp != 1) { rc = 1; snprintf(po_error, sizeof(po_error), "malformed filter tree"); }
  if (rc) { for (int i = 0; i < sp; i++) free(stack[i]); free(stack); return 1; }
  *out_words = stack[0];
  free(stack);
  return 0;
}

/* ------------------------------------------------------------------------------------------------------------------------------
 * numEntriesScannedInFilter, exactly: the reference's BlockDocIdIterator tree restated and driven the way DocIdSetOperator drives
 * it (next() until EOF, core/operator/DocIdSetOperator.java:66-90).  Every ScanBasedDocIdIterator counts the docs whose value it
 * looks at (SVScanDocIdIterator._numEntriesScanned); which docs those are depends on how its parents call it:
 *   SVScanDocIdIterator           next(): 256-doc batches until one holds a match (:76-98); advance(t): doc by doc from t to the
 *                                 first match (:101-112); applyAnd(bitmap): one entry per doc of the bitmap (:115-145)
 *   AndDocIdSet.iterator()        docidsets/AndDocIdSet.java:73-172: index-based children (sorted ranges, bitmaps) are merged, every
 *                                 scan-based child is and-ed into that bitmap with applyAnd in list order, whatever remains (OR / NOT
 *                                 / nested iterators) leap-frogs with the merged bitmap in an AndDocIdIterator; without an
 *                                 index-based child all children leap-frog (dociditerators/AndDocIdIterator.java:41-74)
 *   OrDocIdSet.iterator()         docidsets/OrDocIdSet.java:62-126 -> OrDocIdIterator (dociditerators/OrDocIdIterator.java:52-120)
 *   NotDocIdSet / NotDocIdIterator  docidsets/NotDocIdSet.java:39-41, dociditerators/NotDocIdIterator.java:36-70
 *   getTrues / getFalses          filter/AndFilterOperator.java:52-88, OrFilterOperator.java:51-87, NotFilterOperator.java:52-63,
 *                                 BaseFilterOperator.java:96-113
 * A scan leaf is represented by its match bitmap (the value matcher's answers): the count depends on nothing else.
 * (This fork's OrDocIdSet never fills its bitmapBasedDocIdIterators list, :80-82, so bitmap children of an OR iterate individually
 * whenever nothing is merged -- followed here.  When two or more SORTED children are merged (:98-126) the fork builds the merged
 * iterator from the sorted children alone and the bitmap children are in NO iterator: docs only a posting matches drop out of the OR.
 * That is a bug of the fork, not a semantic: ds_iterator below KNOWINGLY deviates and ors the bitmap children into the merged iterator
 * (what upstream Pinot's filled list does), so the oracle's docId sets are the query's.)
 * ------------------------------------------------------------------------------------------------------------------------------ */
enum { IT_EMPTY = 0, IT_MATCH_ALL, IT_SCAN, IT_SORTED, IT_BITMAP, IT_RANGELESS, IT_AND, IT_OR, IT_NOT };

typedef struct po_it {
  int kind;
  int32_t num_docs;
  /* SCAN / SORTED / BITMAP / RANGELESS: the docId set as dense words (owned iff owns_words) */
  uint64_t* words; int owns_words;
  int64_t pos;                                   /* bitmap iterators: next candidate docId */
  /* SCAN */
  int32_t next_doc_id, first_mismatch, cursor; int32_t batch[PO_SCAN_BATCH]; int64_t* entries;
  /* AND / OR / NOT */
  struct po_it** child; int num_children;
  int32_t next_doc;                              /* AND _nextDocId, NOT _nextDocId, MATCH_ALL _nextDocId */
  int32_t* next_ids; int num_live; int32_t previous;   /* OR */
  int32_t next_non_matching;                     /* NOT */
} po_it;

static int32_t words_next_set(const uint64_t* w, int32_t num_docs, int64_t from) {
  if (from >= num_docs) return PO_EOF;
  int64_t nw = bitmap_words(num_docs), i = from >> 6;
  uint64_t cur = w[i] & (~0ull << (from & 63));
  while (cur == 0) { if (++i >= nw) return PO_EOF; cur = w[i]; }
  int64_t d = i * 64 + __builtin_ctzll(cur);
  return d < num_docs ? (int32_t)d : PO_EOF;
}

static int32_t it_next(po_it* it);
static int32_t it_advance(po_it* it, int32_t target);

static int32_t it_next(po_it* it) {
  switch (it->kind) {
    case IT_EMPTY: return PO_EOF;
    case IT_MATCH_ALL: return it->next_doc < it->num_docs ? it->next_doc++ : PO_EOF;
    case IT_SCAN: {
      if (it->cursor >= it->first_mismatch) {
        int32_t limit, batch_size = 0;
        do {
          limit = it->num_docs - it->next_doc_id;
          if (limit > PO_SCAN_BATCH) limit = PO_SCAN_BATCH;
          if (limit > 0) {
            batch_size = 0;
            for (int32_t i = 0; i < limit; i++) { int32_t d = it->next_doc_id + i; if ((it->words[d >> 6] >> (d & 63)) & 1ull) it->batch[batch_size++] = d; }
            it->next_doc_id += limit;
            *it->entries += limit;
          }
        } while ((limit > 0) & (batch_size == 0));
        it->first_mismatch = batch_size;
        it->cursor = 0;
        if (batch_size == 0) return PO_EOF;
      }
      return it->batch[it->cursor++];
    }
    case IT_SORTED: case IT_BITMAP: case IT_RANGELESS: {
      int32_t d = words_next_set(it->words, it->num_docs, it->pos);
      if (d == PO_EOF) { it->pos = it->num_docs; return PO_EOF; }
      it->pos = (int64_t)d + 1;
      return d;
    }
    case IT_AND: {
      int32_t max_doc = it->next_doc; int max_idx = -1, index = 0;
      while (index < it->num_children) {
        if (index == max_idx) { index++; continue; }
        int32_t d = it_advance(it->child[index], max_doc);
        if (d == PO_EOF) return PO_EOF;
        if (d == max_doc) index++; else { max_doc = d; max_idx = index; index = 0; }
      }
      it->next_doc = max_doc;
      return it->next_doc++;
    }
    case IT_OR: {
      int32_t next = INT32_MAX; int exhausted = 0;
      for (int i = 0; i < it->num_live; i++) {
        int32_t d = it->next_ids[i];
        if (d == it->previous) {
          d = it_next(it->child[i]); it->next_ids[i] = d;
          if (d == PO_EOF) { exhausted = 1; continue; }
        }
        if (d < next) next = d;
      }
      if (exhausted) { int i = 0; while (i < it->num_live) { if (it->next_ids[i] == PO_EOF) { it->num_live--; po_it* gone = it->child[i]; it->child[i] = it->child[it->num_live]; it->child[it->num_live] = gone; it->next_ids[i] = it->next_ids[it->num_live]; it->next_ids[it->num_live] = PO_EOF; } else i++; } }
      if (next != INT32_MAX) { it->previous = next; return next; }
      return PO_EOF;
    }
    default: {   /* IT_NOT */
      if (it->next_doc >= it->num_docs) return PO_EOF;
      while (it->next_doc == it->next_non_matching) {
        it->next_doc++;
        int32_t d = it_next(it->child[0]);
        it->next_non_matching = d == PO_EOF ? it->num_docs : d;
      }
      if (it->next_doc >= it->num_docs) return PO_EOF;
      return it->next_doc++;
    }
  }
}

static int32_t it_advance(po_it* it, int32_t target) {
  switch (it->kind) {
    case IT_EMPTY: return PO_EOF;
    case IT_MATCH_ALL: it->next_doc = target; return it_next(it);
    case IT_SCAN: {
      it->next_doc_id = target; it->first_mismatch = 0;
      while (it->next_doc_id < it->num_docs) {
        int32_t d = it->next_doc_id++;
        (*it->entries)++;
        if ((it->words[d >> 6] >> (d & 63)) & 1ull) return d;
      }
      return PO_EOF;
    }
    case IT_SORTED: case IT_BITMAP: case IT_RANGELESS: if (target > it->pos) it->pos = target; return it_next(it);   /* advanceIfNeeded + next */
    case IT_AND: it->next_doc = target; return it_next(it);
    case IT_OR: {
      int32_t next = INT32_MAX; int exhausted = 0;
      for (int i = 0; i < it->num_live; i++) {
        int32_t d = it->next_ids[i];
        if (d < target) {
          d = it_advance(it->child[i], target); it->next_ids[i] = d;
          if (d == PO_EOF) { exhausted = 1; continue; }
        }
        if (d < next) next = d;
      }
      if (exhausted) { int i = 0; while (i < it->num_live) { if (it->next_ids[i] == PO_EOF) { it->num_live--; po_it* gone = it->child[i]; it->child[i] = it->child[it->num_live]; it->child[it->num_live] = gone; it->next_ids[i] = it->next_ids[it->num_live]; it->next_ids[it->num_live] = PO_EOF; } else i++; } }
      if (next != INT32_MAX) { it->previous = next; return next; }
      return PO_EOF;
    }
    default: {   /* IT_NOT */
      it->next_doc = target;
      if (target > it->next_non_matching) {
        int32_t d = it_advance(it->child[0], target);
        it->next_non_matching = d == PO_EOF ? it->num_docs : d;
      }
      return it_next(it);
    }
  }
}

/* A BlockDocIdSet: what getTrues / getFalses build before anybody asks for an iterator. */
enum { DS_EMPTY = 0, DS_MATCH_ALL, DS_SCAN, DS_SORTED, DS_BITMAP, DS_AND, DS_OR, DS_NOT };
typedef struct po_ds { int kind; uint64_t* words; struct po_ds** child; int num_children; } po_ds;

static po_ds* ds_new(int kind, int nchildren) {
  po_ds* s = (po_ds*)calloc(1, sizeof(po_ds));
  s->kind = kind;
  if (nchildren) s->child = (po_ds**)calloc((size_t)nchildren, sizeof(po_ds*));
  return s;
}
static void ds_free(po_ds* s) { if (!s) return; for (int i = 0; i < s->num_children; i++) ds_free(s->child[i]); free(s->child); free(s->words); free(s); }
static void it_free(po_it* it) {
  if (!it) return;
  for (int i = 0; i < it->num_children; i++) it_free(it->child[i]);
  /* OR swaps exhausted children out of the live prefix but keeps all of them in child[] */
  free(it->child); free(it->next_ids); if (it->owns_words) free(it->words); free(it);
}
static po_it* it_new(int kind, int32_t num_docs) { po_it* it = (po_it*)calloc(1, sizeof(po_it)); it->kind = kind; it->num_docs = num_docs; return it; }

static po_it* ds_iterator(const po_ds* s, int32_t num_docs, int64_t* entries);

/* AndDocIdSet.iterator(), AndDocIdSet.java:73-172 */
static po_it* and_iterator(const po_ds* s, int32_t num_docs, int64_t* entries) {
  int n = s->num_children;
  po_it** all = (po_it**)calloc((size_t)n, sizeof(po_it*));
  int nsorted = 0, nbitmap = 0, nscan = 0, nrem = 0;
  for (int i = 0; i < n; i++) {
    all[i] = ds_iterator(s->child[i], num_docs, entries);
    int k = all[i]->kind;
    if (k == IT_SORTED) nsorted++; else if (k == IT_BITMAP || k == IT_RANGELESS) nbitmap++; else if (k == IT_SCAN) nscan++; else nrem++;
  }
  int64_t nw = bitmap_words(num_docs);
  if ((nsorted + nbitmap > 0 && nscan > 0) || nsorted + nbitmap > 1) {
    uint64_t* docs = (uint64_t*)malloc((size_t)(nw ? nw : 1) * 8);
    memset(docs, 0xFF, (size_t)nw * 8); bitmap_clear_tail(docs, num_docs);
    for (int i = 0; i < n; i++) if (all[i]->kind == IT_SORTED || all[i]->kind == IT_BITMAP || all[i]->kind == IT_RANGELESS) for (int64_t w = 0; w < nw; w++) docs[w] &= all[i]->words[w];
    /* scan-based children in list order (andScanReordering off): ScanBasedDocIdIterator.applyAnd */
    for (int i = 0; i < n; i++) if (all[i]->kind == IT_SCAN) {
      int any = 0;
      for (int64_t w = 0; w < nw; w++) any |= docs[w] != 0;
      if (!any) continue;                                             /* applyAnd: !docIdIterator.hasNext() -> empty, nothing counted */
      for (int64_t w = 0; w < nw; w++) { *entries += __builtin_popcountll(docs[w]); docs[w] &= all[i]->words[w]; }
    }
    po_it* merged = it_new(IT_RANGELESS, num_docs);
    merged->words = docs; merged->owns_words = 1;
    po_it* out = merged;
    if (nrem > 0) {
      out = it_new(IT_AND, num_docs);
      out->child = (po_it**)calloc((size_t)nrem + 1, sizeof(po_it*));
      out->child[out->num_children++] = merged;
      for (int i = 0; i < n; i++) { int k = all[i]->kind; if (k != IT_SORTED && k != IT_BITMAP && k != IT_RANGELESS && k != IT_SCAN) { out->child[out->num_children++] = all[i]; all[i] = NULL; } }
    }
    for (int i = 0; i < n; i++) it_free(all[i]);
    free(all);
    return out;
  }
  po_it* out = it_new(IT_AND, num_docs);
  out->child = all; out->num_children = n;
  return out;
}

static po_it* ds_iterator(const po_ds* s, int32_t num_docs, int64_t* entries) {
  switch (s->kind) {
    case DS_EMPTY: return it_new(IT_EMPTY, num_docs);
    case DS_MATCH_ALL: return it_new(IT_MATCH_ALL, num_docs);
    case DS_SCAN: { po_it* it = it_new(IT_SCAN, num_docs); it->words = s->words; it->entries = entries; return it; }
    case DS_SORTED: { po_it* it = it_new(IT_SORTED, num_docs); it->words = s->words; return it; }
    case DS_BITMAP: { po_it* it = it_new(IT_BITMAP, num_docs); it->words = s->words; return it; }
    case DS_AND: return and_iterator(s, num_docs, entries);
    case DS_OR: {
      /* OrDocIdSet.iterator(): two or more SORTED children are merged into one BitmapDocIdIterator that leads the OrDocIdIterator */
      int n = s->num_children, nsorted = 0;
      po_it* out = it_new(IT_OR, num_docs);
      out->child = (po_it**)calloc((size_t)n + 1, sizeof(po_it*));
      po_it** all = (po_it**)calloc((size_t)n, sizeof(po_it*));
      for (int i = 0; i < n; i++) { all[i] = ds_iterator(s->child[i], num_docs, entries); nsorted += all[i]->kind == IT_SORTED; }
      if (nsorted > 1) {
        int64_t nw = bitmap_words(num_docs);
        po_it* merged = it_new(IT_BITMAP, num_docs);
        merged->words = (uint64_t*)calloc((size_t)(nw ? nw : 1), 8); merged->owns_words = 1;
        for (int i = 0; i < n; i++) if (all[i]->kind == IT_SORTED || all[i]->kind == IT_BITMAP || all[i]->kind == IT_RANGELESS) {
          for (int64_t w = 0; w < nw; w++) merged->words[w] |= all[i]->words[w];     /* (the bitmap children too: see the note above) */
          it_free(all[i]); all[i] = NULL;
        }
        out->child[out->num_children++] = merged;
      }
      for (int i = 0; i < n; i++) if (all[i]) out->child[out->num_children++] = all[i];
      free(all);
      if (out->num_children == 1) { po_it* only = out->child[0]; out->num_children = 0; it_free(out); return only; }
      out->next_ids = (int32_t*)malloc((size_t)out->num_children * 4);
      for (int i = 0; i < out->num_children; i++) out->next_ids[i] = -1;
      out->num_live = out->num_children; out->previous = -1;
      return out;
    }
    default: {   /* DS_NOT: NotDocIdIterator's constructor already pulls the child's first docId */
      po_it* out = it_new(IT_NOT, num_docs);
      out->child = (po_it**)calloc(1, sizeof(po_it*));
      out->child[0] = ds_iterator(s->child[0], num_docs, entries); out->num_children = 1;
      int32_t d = it_next(out->child[0]);
      out->next_non_matching = d == PO_EOF ? num_docs : d;
      return out;
    }
  }
}

static po_ds* ds_trues(const po_column* cols, const pg_segment_desc* seg, const pg_query* q, int node, const int* first_child, int* rc);
static po_ds* ds_falses(const po_column* cols, const pg_segment_desc* seg, const pg_query* q, int node, const int* first_child, int* rc);

/* children of postfix node `node`, left to right: child c ends where child c + 1 starts */
static void node_children(const pg_query* q, int node, const int* start, int* out) {
  int k = q->filter[node].op == PG_FILTER_NOT ? 1 : q->filter[node].num_children;
  int end = node - 1;
  for (int c = k - 1; c >= 0; c--) { out[c] = end; end = start[end] - 1; }
}

static po_ds* ds_leaf(const po_column* cols, const pg_segment_desc* seg, const pg_predicate* p, int* rc) {
  int32_t num_docs = seg->num_docs;
  if (p->kind == PG_PRED_MATCH_ALL || p->kind == PG_PRED_MATCH_NONE) return ds_new(((p->kind == PG_PRED_MATCH_ALL) != (p->exclusive != 0)) ? DS_MATCH_ALL : DS_EMPTY, 0);
  int64_t nw = bitmap_words(num_docs), unused = 0;
  po_ds* s = ds_new(p->kind == PG_PRED_DOC_RANGE ? DS_SORTED : ((p->kind == PG_PRED_IS_NULL || p->eval == PG_EVAL_INVERTED) ? DS_BITMAP : DS_SCAN), 0);
  s->words = (uint64_t*)malloc((size_t)(nw ? nw : 1) * 8);
  if (leaf_to_bitmap(cols, seg, p, s->words, &unused)) *rc = 1;
  return s;
}

static po_ds* ds_trues(const po_column* cols, const pg_segment_desc* seg, const pg_query* q, int node, const int* start, int* rc) {
  const pg_filter_node* fn = &q->filter[node];
  if (fn->op == PG_FILTER_LEAF) return ds_leaf(cols, seg, &q->predicates[fn->predicate], rc);
  int kids[64];
  int k = fn->op == PG_FILTER_NOT ? 1 : fn->num_children;
  if (k > 64) { *rc = 1; return ds_new(DS_EMPTY, 0); }
  node_children(q, node, start, kids);
  if (fn->op == PG_FILTER_NOT) return ds_falses(cols, seg, q, kids[0], start, rc);          /* NotFilterOperator.getTrues */
  po_ds* s = ds_new(fn->op == PG_FILTER_AND ? DS_AND : DS_OR, k);
  for (int c = 0; c < k; c++) s->child[s->num_children++] = ds_trues(cols, seg, q, kids[c], start, rc);
  return s;
}

static po_ds* ds_not(po_ds* inner) { po_ds* s = ds_new(DS_NOT, 1); s->child[0] = inner; s->num_children = 1; return s; }

static po_ds* ds_falses(const po_column* cols, const pg_segment_desc* seg, const pg_query* q, int node, const int* start, int* rc) {
  const pg_filter_node* fn = &q->filter[node];
  if (fn->op == PG_FILTER_LEAF) {                                                          /* BaseFilterOperator.getFalses */
    po_ds* t = ds_leaf(cols, seg, &q->predicates[fn->predicate], rc);
    if (t->kind == DS_MATCH_ALL) { t->kind = DS_EMPTY; return t; }
    if (t->kind == DS_EMPTY) { t->kind = DS_MATCH_ALL; return t; }
    return ds_not(t);
  }
  int kids[64];
  int k = fn->op == PG_FILTER_NOT ? 1 : fn->num_children;
  if (k > 64) { *rc = 1; return ds_new(DS_EMPTY, 0); }
  node_children(q, node, start, kids);
  if (fn->op == PG_FILTER_NOT) return ds_trues(cols, seg, q, kids[0], start, rc);          /* NotFilterOperator.getFalses */
  const int is_and = fn->op == PG_FILTER_AND;
  po_ds* inner = ds_new(is_and ? DS_AND : DS_OR, k);
  for (int c = 0; c < k; c++) {
    po_ds* t = ds_trues(cols, seg, q, kids[c], start, rc);
    /* And: an empty child makes the AND empty, NOT of it everything; match-all children drop out.  Or: the mirror image. */
    if (t->kind == (is_and ? DS_EMPTY : DS_MATCH_ALL)) { ds_free(t); ds_free(inner); return ds_new(is_and ? DS_MATCH_ALL : DS_EMPTY, 0); }
    if (t->kind == (is_and ? DS_MATCH_ALL : DS_EMPTY)) { ds_free(t); continue; }
    inner->child[inner->num_children++] = t;
  }
  if (inner->num_children == 0) { ds_free(inner); return ds_new(is_and ? DS_EMPTY : DS_MATCH_ALL, 0); }
  if (inner->num_children == 1) { po_ds* only = inner->child[0]; inner->num_children = 0; ds_free(inner); return ds_not(only); }
  return ds_not(inner);
}

/* numEntriesScannedInFilter of the filter as the reference would execute it (enableNullHandling off). */
static int filter_entries_scanned(const po_column* cols, const pg_segment_desc* seg, const pg_query* q, int64_t* out_entries) {
  *out_entries = 0;
  int n = q->num_filter_nodes;
  if (n == 0) return 0;
  int* start = (int*)calloc((size_t)n, sizeof(int));
  for (int i = 0; i < n; i++) {
    int k = q->filter[i].op == PG_FILTER_LEAF ? 0 : (q->filter[i].op == PG_FILTER_NOT ? 1 : q->filter[i].num_children);
    int s = i;
    for (int c = 0; c < k; c++) { if (s - 1 < 0) { free(start); PO_FAIL(1, "malformed filter tree"); } s = start[s - 1]; }
    start[i] = s;
  }
  int rc = 0;
  po_ds* root = ds_trues(cols, seg, q, n - 1, start, &rc);
  free(start);
  if (!rc) {
    po_it* it = ds_iterator(root, seg->num_docs, out_entries);
    while (it_next(it) != PO_EOF) {}
    it_free(it);
  }
  ds_free(root);
  return rc;
}

/* Test hook: the iterator objects above driven by a script of calls, the way the reference's own iterator tests drive theirs
 * (dociditerators/NotDocIdIteratorTest.java:31-104: advance(1) = 2, next() = 3, ... over RangelessBitmapDocIdIterators and an
 * OrDocIdIterator of three of them).  A NotDocIdIterator over: kind 0 the bitmap member[0]; kind 1 an OrDocIdIterator of the bitmap
 * members; kind 2 a scan leaf whose matches are member[0] (SVScanDocIdIterator: *out_entries is what it counts).  Kinds 3 and 4: no NOT
 * -- an AndDocIdIterator / an OrDocIdIterator of the bitmap members themselves (AndDocIdIteratorTest.java:32-55, OrDocIdIteratorTest.java:
 * 32-57).  script[i] >= 0: advance(script[i]); -1: next().  out[i] = the docId returned (PO_EOF = the reference's Constants.EOF). */
int po_not_iterator_script(int kind, const uint64_t* const* member_words, int num_members, int32_t num_docs, const int32_t* script, int n, int32_t* out,
                           int64_t* out_entries) {
  if (num_members < 1 || (kind != 1 && kind != 3 && kind != 4 && num_members != 1)) return 1;
  int64_t entries = 0;
  po_ds* inner;
  if (kind == 3) {
    /* (AndDocIdSet.iterator() would merge bitmap children into one bitmap: the test builds the AndDocIdIterator itself, so does this) */
    po_it* it = it_new(IT_AND, num_docs);
    it->child = (po_it**)calloc((size_t)num_members, sizeof(po_it*));
    int64_t nw = bitmap_words(num_docs);
    for (int i = 0; i < num_members; i++) {
      po_it* m = it_new(IT_RANGELESS, num_docs);
      m->words = (uint64_t*)malloc((size_t)(nw ? nw : 1) * 8); m->owns_words = 1;
      memcpy(m->words, member_words[i], (size_t)nw * 8);
      it->child[it->num_children++] = m;
    }
    for (int i = 0; i < n; i++) out[i] = script[i] >= 0 ? it_advance(it, script[i]) : it_next(it);
    it_free(it);
    if (out_entries) *out_entries = 0;
    return 0;
  }
  if (kind == 1 || kind == 4) {
    inner = ds_new(DS_OR, num_members);
    for (int i = 0; i < num_members; i++) {
      po_ds* m = ds_new(DS_BITMAP, 0);
      int64_t nw = bitmap_words(num_docs);
      m->words = (uint64_t*)malloc((size_t)(nw ? nw : 1) * 8);
      memcpy(m->words, member_words[i], (size_t)nw * 8);
      inner->child[inner->num_children++] = m;
    }
  } else {
    inner = ds_new(kind == 2 ? DS_SCAN : DS_BITMAP, 0);
    int64_t nw = bitmap_words(num_docs);
    inner->words = (uint64_t*)malloc((size_t)(nw ? nw : 1) * 8);
    memcpy(inner->words, member_words[0], (size_t)nw * 8);
  }
  po_ds* root = kind == 4 ? inner : ds_not(inner);
  po_it* it = ds_iterator(root, num_docs, &entries);
  for (int i = 0; i < n; i++) out[i] = script[i] >= 0 ? it_advance(it, script[i]) : it_next(it);
  it_free(it);
  ds_free(root);
  if (out_entries) *out_entries = entries;
  return 0;
}

/* BlockDocIdIterator over either one streaming scan leaf (the C2 shape: ScanBasedFilterOperator directly
 * under DocIdSetOperator) or a materialised bitmap (BitmapDocIdIterator), or match-all. */
typedef struct po_doc_iter {
  int kind;                    /* 0 match-all, 1 scan, 2 bitmap */
  int32_t num_docs, next;
  po_scan_iter scan;
  uint64_t* words; int64_t word_idx; uint64_t cur;
} po_doc_iter;

static inline int32_t doc_iter_next(po_doc_iter* it) {
  switch (it->kind) {
    case 0: return it->next < it->num_docs ? it->next++ : PO_EOF;
    case 1: return scan_iter_next(&it->scan);
    default: {
      int64_t nw = bitmap_words(it->num_docs);
      while (it->cur == 0) {
        it->word_idx++;
        if (it->word_idx >= nw) return PO_EOF;
        it->cur = it->words[it->word_idx];
      }
      int b = __builtin_ctzll(it->cur);
      it->cur &= it->cur - 1;
      return (int32_t)(it->word_idx * 64 + b);
    }
  }
}

/* DataFetcher.ColumnValueReader (core/common/DataFetcher.java:335-386) */
static void fetch_dict_ids(const po_column* col, int32_t num_docs, const int32_t* doc_ids, int32_t len, int32_t* out) {
  po_fixedbit_read_dict_ids((const uint8_t*)col->desc->fwd_data, col->desc->bits_per_value, num_docs, doc_ids, len, out);
}
static void fetch_int_values(const po_column* col, int32_t num_docs, const int32_t* doc_ids, int32_t len,
                             int32_t* dict_id_scratch, int32_t* out) {
  if (col->desc->fwd_encoding == PG_FWD_FIXED_BIT_DICT) {
    fetch_dict_ids(col, num_docs, doc_ids, len, dict_id_scratch);
    const uint8_t* dict = (const uint8_t*)col->desc->dict_data;
    /* Dictionary.readIntValues, sspi/index/reader/Dictionary.java:207-211 */
    for (int32_t i = 0; i < len; i++) out[i] = dict_get_int(dict, dict_id_scratch[i]);
  } else {
    /* ForwardIndexReader.readValuesSV default impl, sspi/index/reader/ForwardIndexReader.java:156-162 */
    for (int32_t i = 0; i < len; i++) out[i] = raw_get_int(&col->raw, doc_ids[i]);
  }
}

/* typed value arrays of one block (BlockValSet.getIntValuesSV / getLongValuesSV / getFloatValuesSV / getDoubleValuesSV) */
typedef struct po_values { int32_t* i; int64_t* l; float* f; double* d; } po_values;

/* DataFetcher.ColumnValueReader.read{Int,Long,Float,Double}Values (core/common/DataFetcher.java:335-470): dictionary
 * columns readDictIds then Dictionary.read*Values (typed get per dictId); raw columns ForwardIndexReader.readValuesSV
 * (sspi/index/reader/ForwardIndexReader.java:156-300, typed get per docId).  Fills the array of the stored type. */
static void fetch_stored_values(const po_column* col, int32_t num_docs, const int32_t* doc_ids, int32_t len,
                                int32_t* dict_id_scratch, po_values* out) {
  const pg_column_desc* d = col->desc;
  if (d->stored_type == PG_TYPE_INT) { fetch_int_values(col, num_docs, doc_ids, len, dict_id_scratch, out->i); return; }
  if (d->fwd_encoding == PG_FWD_FIXED_BIT_DICT) {
    fetch_dict_ids(col, num_docs, doc_ids, len, dict_id_scratch);
    const uint8_t* dict = (const uint8_t*)d->dict_data;
    if (d->stored_type == PG_TYPE_LONG) for (int32_t i = 0; i < len; i++) out->l[i] = dict_get_long(dict, dict_id_scratch[i]);
    else if (d->stored_type == PG_TYPE_FLOAT) for (int32_t i = 0; i < len; i++) out->f[i] = dict_get_float(dict, dict_id_scratch[i]);
    else for (int32_t i = 0; i < len; i++) out->d[i] = dict_get_double(dict, dict_id_scratch[i]);
  } else {
    if (d->stored_type == PG_TYPE_LONG) for (int32_t i = 0; i < len; i++) out->l[i] = raw_get_long(&col->raw, doc_ids[i]);
    else if (d->stored_type == PG_TYPE_FLOAT) for (int32_t i = 0; i < len; i++) out->f[i] = raw_get_float(&col->raw, doc_ids[i]);
    else for (int32_t i = 0; i < len; i++) out->d[i] = raw_get_double(&col->raw, doc_ids[i]);
  }
}
/* getDoubleValuesSV on any numeric stored type: Dictionary.readDoubleValues / readValuesSV(double[]) widen per value */
static void widen_to_double(int stored_type, const po_values* v, int32_t len, double* out) {
  switch (stored_type) {
    case PG_TYPE_INT: for (int32_t i = 0; i < len; i++) out[i] = (double)v->i[i]; break;
    case PG_TYPE_LONG: for (int32_t i = 0; i < len; i++) out[i] = (double)v->l[i]; break;
    case PG_TYPE_FLOAT: for (int32_t i = 0; i < len; i++) out[i] = (double)v->f[i]; break;
    default: for (int32_t i = 0; i < len; i++) out[i] = v->d[i]; break;
  }
}
/* java.lang.Math.max / min on floating point: NaN wins, -0.0 < +0.0 */
static inline double java_max(double a, double b) { if (a != a) return a; if (b != b) return b; if (a == 0.0 && b == 0.0) return signbit(a) ? b : a; return a > b ? a : b; }
static inline double java_min(double a, double b) { if (a != a) return a; if (b != b) return b; if (a == 0.0 && b == 0.0) return signbit(a) ? a : b; return a < b ? a : b; }
static inline float java_maxf(float a, float b) { return (float)java_max((double)a, (double)b); }
static inline float java_minf(float a, float b) { return (float)java_min((double)a, (double)b); }

typedef struct po_holder {          /* DoubleAggregationResultHolder / AvgPair + exact side channel */
  double value;                     /* COUNT, SUM, MIN, MAX holder */
  double avg_sum; int64_t avg_count;
  int64_t exact_sum; int64_t n;
  int overflow;                     /* the int64 side channel wrapped: sum_exact = 0 */
} po_holder;
/* exact integer side channel: wrapping add that remembers whether it ever wrapped */
static inline void exact_add(int64_t* acc, int64_t v, int* overflow) {
  int64_t r;
  if (__builtin_add_overflow(*acc, v, &r)) *overflow = 1;
  *acc = r;
}

static void holder_init(po_holder* h, int func) {
  memset(h, 0, sizeof(*h));
  if (func == PG_AGG_MIN) h->value = INFINITY;
  if (func == PG_AGG_MAX) h->value = -INFINITY;
}

/* One aggregate() call of a function over values[from, to) of a block (the reducer body that foldNotNull applies to each non-null range,
 * NullableSingleInputAggregationFunction.java:118-160; the whole block [0, length) when there are no nulls). */
/* A raw group key as the tuple of its digits (dictIds; value - min of a raw column), group-by column order: what ArrayMapBasedHolder keys
 * by (an IntArray, DictionaryBasedGroupKeyGenerator.java:808+).  The int / long raw key of the narrower holders is its mixed-radix value
 * sum d[j] * prod_{k<j} cardinality_k (:437-445, :650-660); rows are ordered by that value, i.e. the LAST column is the most significant. */
typedef struct po_key { int32_t d[PO_MAX_GROUP_COLS]; } po_key;
static __thread const po_key* po_sort_keys;
static __thread int po_sort_ng;
static int po_key_cmp(const po_key* a, const po_key* b, int ng) {
  for (int c = ng - 1; c >= 0; c--) if (a->d[c] != b->d[c]) return a->d[c] < b->d[c] ? -1 : 1;
  return 0;
}
static int po_cmp_by_key(const void* a, const void* b) {
  return po_key_cmp(&po_sort_keys[*(const int32_t*)a], &po_sort_keys[*(const int32_t*)b], po_sort_ng);
}
static uint64_t po_key_value(const po_key* k, const int32_t* cards, int ng) {      /* the int / long raw key (key kinds 0 and 1) */
  uint64_t raw = 0;
  for (int c = ng - 1; c >= 0; c--) raw = raw * (uint64_t)cards[c] + (uint64_t)k->d[c];
  return raw;
}

static int agg_range(po_holder* h, int func, int st, const po_values* vals, int32_t from, int32_t to, double* dbl_values) {
  if (to <= from) return 0;
  switch (func) {
          case PG_AGG_SUM: {
            /* SumAggregationFunction.aggregate :69-129 (one case per stored type, double innerSum), updateAggregationResultHolder :147-157 */
            double inner_sum = 0;
            if (st == PG_TYPE_INT) for (int32_t i = from; i < to; i++) { inner_sum += vals->i[i]; exact_add(&h->exact_sum, vals->i[i], &h->overflow); }
            else if (st == PG_TYPE_LONG) for (int32_t i = from; i < to; i++) { inner_sum += (double)vals->l[i]; exact_add(&h->exact_sum, vals->l[i], &h->overflow); }
            else if (st == PG_TYPE_FLOAT) for (int32_t i = from; i < to; i++) inner_sum += (double)vals->f[i];
            else for (int32_t i = from; i < to; i++) inner_sum += vals->d[i];
            h->value = inner_sum + h->value;
            break;
          }
          case PG_AGG_MAX: {
            /* MaxAggregationFunction.aggregate :69-149 (typed inner max, Math.max), :150-160 */
            double inner;
            if (st == PG_TYPE_INT) { int32_t m = vals->i[from]; for (int32_t i = from; i < to; i++) m = vals->i[i] > m ? vals->i[i] : m; inner = (double)m; }
            else if (st == PG_TYPE_LONG) { int64_t m = vals->l[from]; for (int32_t i = from; i < to; i++) m = vals->l[i] > m ? vals->l[i] : m; inner = (double)m; }
            else if (st == PG_TYPE_FLOAT) { float m = vals->f[from]; for (int32_t i = from; i < to; i++) m = java_maxf(m, vals->f[i]); inner = (double)m; }
            else { double m = vals->d[from]; for (int32_t i = from; i < to; i++) m = java_max(m, vals->d[i]); inner = m; }
            h->value = java_max(inner, h->value);
            break;
          }
          case PG_AGG_MIN: {
            double inner;
            if (st == PG_TYPE_INT) { int32_t m = vals->i[from]; for (int32_t i = from; i < to; i++) m = vals->i[i] < m ? vals->i[i] : m; inner = (double)m; }
            else if (st == PG_TYPE_LONG) { int64_t m = vals->l[from]; for (int32_t i = from; i < to; i++) m = vals->l[i] < m ? vals->l[i] : m; inner = (double)m; }
            else if (st == PG_TYPE_FLOAT) { float m = vals->f[from]; for (int32_t i = from; i < to; i++) m = java_minf(m, vals->f[i]); inner = (double)m; }
            else { double m = vals->d[from]; for (int32_t i = from; i < to; i++) m = java_min(m, vals->d[i]); inner = m; }
            h->value = java_min(inner, h->value);
            break;
          }
          case PG_AGG_AVG: {
            /* AvgAggregationFunction.aggregate :63-79: getDoubleValuesSV, avgPair.apply(v, 1) per doc,
             * then updateAggregationResult -> holder pair.apply(sum, count) :95-102 */
            widen_to_double(st, vals, to, dbl_values);
            double s = 0; int64_t c = 0;
            for (int32_t i = from; i < to; i++) { s += dbl_values[i]; c += 1; }
            if (st == PG_TYPE_INT) for (int32_t i = from; i < to; i++) exact_add(&h->exact_sum, vals->i[i], &h->overflow);
            if (st == PG_TYPE_LONG) for (int32_t i = from; i < to; i++) exact_add(&h->exact_sum, vals->l[i], &h->overflow);
            h->avg_sum += s; h->avg_count += c;
            break;
          }
          default: snprintf(po_error, sizeof(po_error), "unsupported aggregation %d", func); return 2;
        }
  h->n += to - from;
  return 0;
}

/* Folds a per-block holder into the query holder: updateAggregationResultHolder of Sum :147-157 / Min / Max, AvgPair.apply. */
static void holder_merge(po_holder* h, const po_holder* b, int func) {
  if (b->n == 0) return;
  if (func == PG_AGG_SUM) h->value = b->value + h->value;
  if (func == PG_AGG_MIN) h->value = java_min(b->value, h->value);
  if (func == PG_AGG_MAX) h->value = java_max(b->value, h->value);
  if (func == PG_AGG_AVG) { h->avg_sum += b->avg_sum; h->avg_count += b->avg_count; }
  exact_add(&h->exact_sum, b->exact_sum, &h->overflow);
  h->overflow |= b->overflow;
  h->n += b->n;
}

/* Order-preserving 64-bit image of a raw value: INT / LONG v ^ 2^63; FLOAT (widened exactly) / DOUBLE in Double.compare's order (-0.0 below
 * 0.0, every NaN the one canonical NaN above +Infinity: fastutil's Double2IntOpenHashMap keys by doubleToLongBits).  The digit of a raw
 * FLOAT / DOUBLE / wide INT / LONG group-by column is the rank of its image among the column's distinct images (po_execute). */
static uint64_t rank_order_image(const po_column* c, int32_t doc) {
  const int t = c->desc->stored_type;
  if (t == PG_TYPE_INT) return (uint64_t)(int64_t)raw_get_int(&c->raw, doc) ^ (1ull << 63);
  if (t == PG_TYPE_LONG) return (uint64_t)raw_get_long(&c->raw, doc) ^ (1ull << 63);
  double v = t == PG_TYPE_FLOAT ? (double)raw_get_float(&c->raw, doc) : raw_get_double(&c->raw, doc);
  uint64_t b;
  memcpy(&b, &v, 8);
  if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) b = 0x7FF8000000000000ull;
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
static int cmp_u64(const void* a, const void* b) { const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b; return x < y ? -1 : (x > y ? 1 : 0); }

int po_execute(const pg_segment_desc* seg, const pg_query* q, pg_result* res) {
  uint64_t* rank_dict[PO_MAX_GROUP_COLS] = {0};       /* raw FLOAT / DOUBLE / wide key columns: the distinct order images, ascending */
  memset(res, 0, sizeof(*res));
  if (seg->num_docs < 0) PO_FAIL(1, "negative num_docs");
  int32_t num_docs = seg->num_docs;
  po_column* cols = (po_column*)calloc((size_t)(seg->num_columns > 0 ? seg->num_columns : 1), sizeof(po_column));
  for (int32_t c = 0; c < seg->num_columns; c++) {
    cols[c].desc = &seg->columns[c];
    if (seg->columns[c].stored_type < PG_TYPE_INT || seg->columns[c].stored_type > PG_TYPE_DOUBLE) { free(cols); PO_FAIL(2, "oracle: stored type %d is not restated", seg->columns[c].stored_type); }
    if (seg->columns[c].fwd_encoding == PG_FWD_RAW_FIXED_BYTE) {
      if (po_raw_open((const uint8_t*)seg->columns[c].fwd_data, seg->columns[c].fwd_size, &cols[c].raw)) { free(cols); return 1; }
    }
  }
  /* AggregationPlanNode.buildNonFilteredAggOperator (core/plan/AggregationPlanNode.java:98-115): when the filter matches all docs
   * and every function is COUNT or a dictionary-based MIN / MAX (isFitForNonScanBasedPlan :159-190), NonScanBasedAggregationOperator
   * answers from the metadata and the dictionary ends (NonScanBasedAggregationOperator.java:83-105) with statistics
   * (totalDocs, 0, 0, totalDocs). */
  const int null_handling = (q->flags & PG_QUERY_NULL_HANDLING) != 0;
  /* per aggregation: the null bitmap of its column when null handling is on and the column has null docs, else NULL */
  uint64_t** agg_nulls = NULL;
  int has_null_values = 0;                    /* AggregationPlanNode.hasNullValues :130-152 */
  if (null_handling && q->num_aggregations > 0) {
    agg_nulls = (uint64_t**)calloc((size_t)q->num_aggregations, sizeof(uint64_t*));
    for (int a = 0; a < q->num_aggregations; a++) {
      agg_nulls[a] = column_null_words(seg, q->aggregations[a].column);
      has_null_values |= agg_nulls[a] != NULL;
    }
  }
  if (q->num_group_by == 0 && q->num_aggregations > 0 && !has_null_values) {
    int match_all = q->num_filter_nodes == 0;
    if (q->num_filter_nodes == 1 && q->filter[0].op == PG_FILTER_LEAF) {
      const pg_predicate* p = &q->predicates[q->filter[0].predicate];
      match_all = (p->kind == PG_PRED_MATCH_ALL && !p->exclusive) || (p->kind == PG_PRED_MATCH_NONE && p->exclusive);
    }
    int fit = match_all;
    for (int a = 0; a < q->num_aggregations && fit; a++) {
      int func = q->aggregations[a].function, c = q->aggregations[a].column;
      if (func == PG_AGG_COUNT) continue;
      fit = (func == PG_AGG_MIN || func == PG_AGG_MAX) && c >= 0 && c < seg->num_columns && seg->columns[c].fwd_encoding == PG_FWD_FIXED_BIT_DICT;
    }
    if (fit) {
      int na0 = q->num_aggregations;
      res->num_aggregations = na0;
      res->aggregations = (pg_agg_value*)calloc((size_t)na0, sizeof(pg_agg_value));
      for (int a = 0; a < na0; a++) {
        pg_agg_value* v = &res->aggregations[a];
        int func = q->aggregations[a].function;
        v->count = num_docs; v->min = INFINITY; v->max = -INFINITY;
        if (func == PG_AGG_MIN || func == PG_AGG_MAX) {
          const pg_column_desc* d = &seg->columns[q->aggregations[a].column];
          const uint8_t* dict = (const uint8_t*)d->dict_data;
          int32_t id = func == PG_AGG_MIN ? 0 : d->cardinality - 1;       /* dictionary.getMinVal() / getMaxVal() */
          double val = d->stored_type == PG_TYPE_INT ? (double)dict_get_int(dict, id) : d->stored_type == PG_TYPE_LONG ? (double)dict_get_long(dict, id)
                     : d->stored_type == PG_TYPE_FLOAT ? (double)dict_get_float(dict, id) : dict_get_double(dict, id);
          if (func == PG_AGG_MIN) v->min = val; else v->max = val;
        }
      }
      res->stats.num_docs_scanned = num_docs;
      res->stats.num_total_docs = num_docs;
      free(cols); free(agg_nulls);
      return 0;
    }
  }
  int rc = 0;
  int64_t entries_in_filter = 0;
  po_doc_iter* it = (po_doc_iter*)calloc(1, sizeof(po_doc_iter));
  it->num_docs = num_docs;
  uint64_t* filter_words = NULL;
  /* FilterPlanNode: a single scan leaf streams; anything else is materialised (same docId set). */
  if (q->num_filter_nodes == 0) {
    it->kind = 0;
  } else if (!null_handling && q->num_filter_nodes == 1 && q->filter[0].op == PG_FILTER_LEAF &&
             q->predicates[q->filter[0].predicate].eval == PG_EVAL_SCAN &&
             ((q->predicates[q->filter[0].predicate].kind >= PG_PRED_DICT_RANGE &&
               q->predicates[q->filter[0].predicate].kind <= PG_PRED_RAW_RANGE) || q->predicates[q->filter[0].predicate].kind == PG_PRED_RAW_SET)) {
    it->kind = 1;
    const pg_predicate* p = &q->predicates[q->filter[0].predicate];
    scan_iter_init(&it->scan, &cols[p->column], p, num_docs);
  } else {
    if (filter_to_bitmap(cols, seg, q, &filter_words, &entries_in_filter)) {
      if (agg_nulls) for (int a = 0; a < q->num_aggregations; a++) free(agg_nulls[a]);
      free(agg_nulls); free(cols); free(it); return 1;
    }
    /* the docId set came from the set algebra above; the entries scanned come from the reference's iterators */
    if (!null_handling && filter_entries_scanned(cols, seg, q, &entries_in_filter)) {
      if (agg_nulls) for (int a = 0; a < q->num_aggregations; a++) free(agg_nulls[a]);
      free(agg_nulls); free(cols); free(it); free(filter_words); return 1;
    }
    it->kind = 2; it->words = filter_words; it->word_idx = 0; it->cur = bitmap_words(num_docs) ? filter_words[0] : 0;
    if (bitmap_words(num_docs) == 0) it->word_idx = 0;
  }

  int na = q->num_aggregations;
  int ng = q->num_group_by;
  int64_t group_upper = 1;
  unsigned __int128 wide_upper = 1;   /* the product of the cardinalities, saturating at 2^100 (only compared with Integer / Long.MAX_VALUE) */
  int key_kind = 0;               /* 0 int raw keys, 1 long (LongMapBasedHolder), 2 beyond a long (ArrayMapBasedHolder) */
  int32_t cards[PO_MAX_GROUP_COLS];
  uint64_t* key_nulls[PO_MAX_GROUP_COLS] = {0};
  int nullable_group_by = 0;      /* null handling with nulls in a key or an aggregated column: the no-dictionary generators' semantics */
  if (ng > PO_MAX_GROUP_COLS) { rc = 2; snprintf(po_error, sizeof(po_error), "too many group-by columns"); goto done; }
  int64_t key_base[PO_MAX_GROUP_COLS] = {0};
  int key_raw[PO_MAX_GROUP_COLS] = {0};      /* 1: digit = value - min; 2: digit = rank among the column's distinct values */
  int no_dict_keys = 0;           /* a key column without a dictionary: NoDictionarySingle / MultiColumnGroupKeyGenerator */
  for (int g = 0; g < ng; g++) {
    const pg_column_desc* d = &seg->columns[q->group_by_columns[g]];
    cards[g] = d->cardinality;
    if (d->fwd_encoding != PG_FWD_FIXED_BIT_DICT) {
      /* DefaultGroupByExecutor.java:106-121: one key column without a dictionary sends the whole query to the no-dictionary generators,
       * which key by VALUE -- value -> group id in order of first appearance (NoDictionarySingleColumnGroupKeyGenerator.java:100-113,
       * 240-247; NoDictionaryMultiColumnGroupKeyGenerator: the tuple of values / dictIds), _globalGroupIdUpperBound = numGroupsLimit
       * (:73-79).  Restated on the raw-key scale of the ABI (include/pinot_gpu.h, pg_group_key_info): the column's digit is
       * value - min, its digit count max - min + 1; INT / LONG columns whose range fits an int. */
      const po_column* kc = &cols[q->group_by_columns[g]];
      const int integral = d->stored_type == PG_TYPE_INT || d->stored_type == PG_TYPE_LONG;
      int64_t lo = INT64_MAX, hi = INT64_MIN;
      for (int32_t doc = 0; integral && doc < num_docs; doc++) {
        const int64_t v = d->stored_type == PG_TYPE_INT ? (int64_t)raw_get_int(&kc->raw, doc) : raw_get_long(&kc->raw, doc);
        if (v < lo) lo = v;
        if (v > hi) hi = v;
      }
      if (num_docs <= 0) { rc = 2; snprintf(po_error, sizeof(po_error), "group-by on a raw column of an empty segment"); goto done; }
      if (integral && (uint64_t)hi - (uint64_t)lo < 0x7FFFFFFEull) {      /* (unsigned: a LONG column may span more than 2^63) */
        key_base[g] = lo; key_raw[g] = 1; cards[g] = (int32_t)(hi - lo + 1); no_dict_keys = 1;
      } else {
        /* FLOAT / DOUBLE values, INT / LONG values over more than an int: NoDictionarySingleColumnGroupKeyGenerator.java:100-135 keys them by
         * value all the same (Float / Double / Long2IntOpenHashMap).  On the ABI's raw-key scale the column's digit is the value's RANK
         * among the column's distinct values, ascending in Double.compare's / Long.compare's order (include/pinot_gpu.h,
         * pg_group_key_info: *out_is_offset = 2, pg_group_key_values) -- an order-preserving 64-bit image per doc, sorted, deduplicated. */
        if (null_handling) { rc = 2; snprintf(po_error, sizeof(po_error), "group-by on a raw FLOAT / DOUBLE / wide column under null handling"); goto done; }
        uint64_t* img = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)num_docs);
        for (int32_t doc = 0; doc < num_docs; doc++) img[doc] = rank_order_image(kc, doc);
        rank_dict[g] = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)num_docs);
        memcpy(rank_dict[g], img, sizeof(uint64_t) * (size_t)num_docs);
        free(img);
        qsort(rank_dict[g], (size_t)num_docs, sizeof(uint64_t), cmp_u64);
        int64_t c = 0;
        for (int32_t i = 0; i < num_docs; i++) if (i == 0 || rank_dict[g][i] != rank_dict[g][c - 1]) rank_dict[g][c++] = rank_dict[g][i];
        if (c >= 0x7FFFFFFEll) { rc = 2; snprintf(po_error, sizeof(po_error), "group-by on raw column: too many distinct values"); goto done; }
        key_raw[g] = 2; cards[g] = (int32_t)c; no_dict_keys = 1;
      }
    }
    /* DictionaryBasedGroupKeyGenerator.java:150-184: ArrayBasedHolder up to arrayBasedThreshold, IntMapBasedHolder while the product
     * fits an int, LongMapBasedHolder while it fits a long (:628-700), ArrayMapBasedHolder beyond (:808+).  The three map-based holders
     * differ in the key type only: group ids in order of first appearance, new keys refused once the map holds
     * _globalGroupIdUpperBound of them -- min(product, numGroupsLimit) for the int holder, numGroupsLimit for the other two.  One
     * key type -- the digit tuple, po_key -- restates all of them. */
    {
      const unsigned __int128 sat = (unsigned __int128)1 << 100, card = (unsigned __int128)(cards[g] > 0 ? cards[g] : 1);
      wide_upper = (wide_upper >= sat || wide_upper * card >= sat) ? sat : wide_upper * card;
    }
    if (null_handling) {
      /* DefaultGroupByExecutor.java:106-121: under null handling the keys come from the no-dictionary generators
       * (NoDictionarySingleColumnGroupKeyGenerator / NoDictionaryMultiColumnGroupKeyGenerator with nullHandlingEnabled): a null key value
       * is a key of its own, group ids are handed out in order of first appearance up to numGroupsLimit.  Restated on the raw-key
       * scale of the ABI: a nullable key column has one more digit value, `cardinality`, meaning NULL. */
      key_nulls[g] = column_null_words(seg, q->group_by_columns[g]);
      if (key_nulls[g]) { const int32_t card0 = cards[g]; cards[g] = card0 + 1; if (wide_upper < ((unsigned __int128)1 << 100)) wide_upper = wide_upper / (unsigned __int128)(card0 > 0 ? card0 : 1) * (unsigned __int128)cards[g]; nullable_group_by = 1; }
    }
  }
  key_kind = wide_upper > (unsigned __int128)0x7FFFFFFFFFFFFFFFull ? 2 : (wide_upper > (unsigned __int128)2147483647 ? 1 : 0);
  if (key_kind != 0 && null_handling) { rc = 2; snprintf(po_error, sizeof(po_error), "group-by key space beyond an int under null handling"); goto done; }
  group_upper = key_kind == 0 ? (int64_t)wide_upper : 0x7FFFFFFFll;      /* (only an upper bound for the map-based sizing below) */
  if (null_handling && ng > 0 && has_null_values) nullable_group_by = 1;
  if (no_dict_keys && key_kind == 0) nullable_group_by = 1;      /* the same generators: ids by first appearance up to numGroupsLimit whatever the key space */

  /* IntMapBasedHolder (DictionaryBasedGroupKeyGenerator.java:415-490) + IntGroupIdMap.getGroupId (:1022-1047): raw key -> group id in
   * order of first appearance; once _size == groupIdUpperBound = min(product, numGroupsLimit) (:176) new keys get INVALID_ID and the
   * result holders ignore their docs. */
  const int map_based = ng > 0 && (group_upper > 10000 || nullable_group_by);
  const int64_t raw_key_upper = group_upper;
  int32_t num_groups_limit = q->num_groups_limit > 0 ? q->num_groups_limit : 100000;
  int64_t map_capacity = 0; po_key* map_keys = NULL; uint8_t* map_used = NULL; int32_t* map_ids = NULL; po_key* raw_of_gid = NULL; int32_t map_size = 0;
  if (map_based) {
    group_upper = group_upper < num_groups_limit ? group_upper : num_groups_limit;     /* _globalGroupIdUpperBound */
    map_capacity = 16; while (map_capacity < 2 * group_upper + 2) map_capacity <<= 1;
    map_keys = (po_key*)malloc(sizeof(po_key) * (size_t)map_capacity);
    map_used = (uint8_t*)calloc((size_t)map_capacity, 1);
    map_ids = (int32_t*)malloc(sizeof(int32_t) * (size_t)map_capacity);
    raw_of_gid = (po_key*)malloc(sizeof(po_key) * (size_t)(group_upper > 0 ? group_upper : 1));
  }

  po_holder* holders = NULL;       /* aggregation only */
  double* gholders = NULL;         /* group-by: [na][G] DoubleGroupByResultHolder */
  double* gavg_sum = NULL; int64_t* gavg_cnt = NULL; int64_t* gexact = NULL; int64_t* gcount = NULL; int* gover = NULL;
  uint8_t* flags = NULL;
  if (ng == 0) {
    holders = (po_holder*)calloc((size_t)(na > 0 ? na : 1), sizeof(po_holder));
    for (int a = 0; a < na; a++) holder_init(&holders[a], q->aggregations[a].function);
  } else {
    size_t G = (size_t)group_upper;
    gholders = (double*)malloc(sizeof(double) * G * (size_t)(na > 0 ? na : 1));
    gavg_sum = (double*)calloc(G * (size_t)(na > 0 ? na : 1), sizeof(double));
    gavg_cnt = (int64_t*)calloc(G * (size_t)(na > 0 ? na : 1), sizeof(int64_t));
    gexact = (int64_t*)calloc(G * (size_t)(na > 0 ? na : 1), sizeof(int64_t));
    gover = (int*)calloc(G * (size_t)(na > 0 ? na : 1), sizeof(int));
    gcount = (int64_t*)calloc(G, sizeof(int64_t));
    flags = (uint8_t*)calloc(G, 1);
    for (int a = 0; a < na; a++) {
      double init = q->aggregations[a].function == PG_AGG_MIN ? INFINITY : (q->aggregations[a].function == PG_AGG_MAX ? -INFINITY : 0.0);
      for (size_t g = 0; g < G; g++) gholders[(size_t)a * G + g] = init;
    }
  }

  /* thread-local scratch of the reference: DocIdSetOperator.java:42-43, DataFetcher.java:50-51 */
  int32_t* doc_ids = (int32_t*)malloc(sizeof(int32_t) * PO_MAX_DOC_PER_CALL);
  int32_t* dict_scratch = (int32_t*)malloc(sizeof(int32_t) * PO_MAX_DOC_PER_CALL);
  po_values vals;
  vals.i = (int32_t*)malloc(sizeof(int32_t) * PO_MAX_DOC_PER_CALL);
  vals.l = (int64_t*)malloc(sizeof(int64_t) * PO_MAX_DOC_PER_CALL);
  vals.f = (float*)malloc(sizeof(float) * PO_MAX_DOC_PER_CALL);
  vals.d = (double*)malloc(sizeof(double) * PO_MAX_DOC_PER_CALL);
  double* dbl_values = (double*)malloc(sizeof(double) * PO_MAX_DOC_PER_CALL);
  int32_t* group_ids = (int32_t*)malloc(sizeof(int32_t) * PO_MAX_DOC_PER_CALL);
  po_key* raw_keys = (po_key*)malloc(sizeof(po_key) * PO_MAX_DOC_PER_CALL);
  int32_t* nn_gids = (int32_t*)malloc(sizeof(int32_t) * PO_MAX_DOC_PER_CALL);
  int64_t* gnn = ng > 0 ? (int64_t*)calloc((size_t)group_upper * (size_t)(na > 0 ? na : 1), sizeof(int64_t)) : NULL;   /* docs that reached the holder, per group and function */
  int64_t num_docs_scanned = 0;

  for (;;) {
    /* DocIdSetOperator.getNextBlock, core/operator/DocIdSetOperator.java:72-85 */
    int32_t pos = 0;
    for (int32_t i = 0; i < PO_MAX_DOC_PER_CALL; i++) {
      int32_t d = doc_iter_next(it);
      if (d == PO_EOF) break;
      doc_ids[pos++] = d;
    }
    if (pos == 0) break;
    num_docs_scanned += pos;

    if (ng > 0) {
      /* DictionaryBasedGroupKeyGenerator.ArrayBasedHolder.processSingleValue, :298-338 */
      for (int g = ng - 1; g >= 0; g--) {
        if (key_raw[g] == 2) {
          const po_column* kc = &cols[q->group_by_columns[g]];
          for (int32_t i = 0; i < pos; i++) {
            const uint64_t key = rank_order_image(kc, doc_ids[i]);
            int32_t lo = 0, hi = cards[g] - 1;
            while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (rank_dict[g][mid] < key) lo = mid + 1; else hi = mid; }
            dict_scratch[i] = lo;
          }
        } else if (key_raw[g]) {
          const po_column* kc = &cols[q->group_by_columns[g]];
          const int is_int = kc->desc->stored_type == PG_TYPE_INT;
          for (int32_t i = 0; i < pos; i++) dict_scratch[i] = (int32_t)((is_int ? (int64_t)raw_get_int(&kc->raw, doc_ids[i]) : raw_get_long(&kc->raw, doc_ids[i])) - key_base[g]);
        } else fetch_dict_ids(&cols[q->group_by_columns[g]], num_docs, doc_ids, pos, dict_scratch);
        if (key_nulls[g]) for (int32_t i = 0; i < pos; i++) if ((key_nulls[g][doc_ids[i] >> 6] >> (doc_ids[i] & 63)) & 1) dict_scratch[i] = cards[g] - 1;   /* NULL */
        for (int32_t i = 0; i < pos; i++) raw_keys[i].d[g] = dict_scratch[i];
      }
      if (!map_based) for (int32_t i = 0; i < pos; i++) group_ids[i] = (int32_t)po_key_value(&raw_keys[i], cards, ng);
      if (map_based) {
        /* group ids in first-appearance order; docs of keys refused by the full map drop out of every aggregation (the holders
         * ignore INVALID_ID) but still count as scanned */
        int32_t kept = 0;
        for (int32_t i = 0; i < pos; i++) {
          const po_key raw = raw_keys[i];
          uint64_t h = 0;
          for (int c = 0; c < ng; c++) h = (h ^ (uint64_t)(uint32_t)raw.d[c]) * 0x9E3779B97F4A7C15ull + 0xC2B2AE3D27D4EB4Full;
          h >>= 20;
          int64_t slot = (int64_t)(h & (uint64_t)(map_capacity - 1));
          int32_t gid = -1;
          for (;;) {
            if (map_used[slot] && po_key_cmp(&map_keys[slot], &raw, ng) == 0) { gid = map_ids[slot]; break; }
            if (!map_used[slot]) {
              if (map_size < group_upper) { map_used[slot] = 1; map_keys[slot] = raw; map_ids[slot] = map_size; raw_of_gid[map_size] = raw; gid = map_size++; }
              break;
            }
            slot = (slot + 1) & (map_capacity - 1);
          }
          if (gid < 0) continue;
          doc_ids[kept] = doc_ids[i]; group_ids[kept] = gid; kept++;
        }
        /* (num_docs_scanned already holds the whole block: GroupByOperator.java:111) */
        pos = kept;
        if (pos == 0) continue;
      }
      for (int32_t i = 0; i < pos; i++) { flags[group_ids[i]] = 1; gcount[group_ids[i]]++; }
    }

    for (int a = 0; a < na; a++) {
      int func = q->aggregations[a].function;
      int colidx = q->aggregations[a].column;
      size_t G = (size_t)group_upper;
      if (func == PG_AGG_COUNT) {
        if (ng == 0) {
          /* CountAggregationFunction.aggregate :84-88; COUNT(column) under null handling counts length - numNulls (:88-97) */
          int32_t num_nulls = 0;
          if (agg_nulls && agg_nulls[a]) for (int32_t i = 0; i < pos; i++) num_nulls += (int32_t)((agg_nulls[a][doc_ids[i] >> 6] >> (doc_ids[i] & 63)) & 1);
          holders[a].value = holders[a].value + (pos - num_nulls);
        } else {
          /* aggregateGroupBySV :110-116; COUNT(column) under null handling skips the null docs (:118-131) */
          for (int32_t i = 0; i < pos; i++) {
            if (agg_nulls && agg_nulls[a] && ((agg_nulls[a][doc_ids[i] >> 6] >> (doc_ids[i] & 63)) & 1)) continue;
            gholders[(size_t)a * G + group_ids[i]] = gholders[(size_t)a * G + group_ids[i]] + 1;
          }
        }
        continue;
      }
      if (colidx < 0 || colidx >= seg->num_columns) { rc = 1; snprintf(po_error, sizeof(po_error), "bad aggregation column"); goto cleanup; }
      const int st = cols[colidx].desc->stored_type;
      fetch_stored_values(&cols[colidx], num_docs, doc_ids, pos, dict_scratch, &vals);
      if (ng == 0) {
        po_holder* h = &holders[a];
        if (agg_nulls && agg_nulls[a]) {
          /* foldNotNull / forEachNotNull (NullableSingleInputAggregationFunction.java:72-160): the reducer runs on every maximal range of
           * non-null positions of the block, then the block result is folded into the holder (nothing when the block is all null). */
          po_holder blk; holder_init(&blk, func);
          int32_t from = 0;
          for (int32_t i = 0; i <= pos && !rc; i++) {
            const int is_null = i < pos && ((agg_nulls[a][doc_ids[i] >> 6] >> (doc_ids[i] & 63)) & 1);
            if (i == pos || is_null) { rc = agg_range(&blk, func, st, &vals, from, i, dbl_values); from = i + 1; }
          }
          if (rc) goto cleanup;
          holder_merge(h, &blk, func);
        } else {
          rc = agg_range(h, func, st, &vals, 0, pos, dbl_values);
          if (rc) goto cleanup;
        }
      } else {
        /* group-by functions all read getDoubleValuesSV (Dictionary.readDoubleValues / readValuesSV(double[])) */
        widen_to_double(st, &vals, pos, dbl_values);
        double* hold = gholders + (size_t)a * G;
        int64_t* ex = gexact + (size_t)a * G;
        const int32_t* gids = group_ids;
        int32_t npos = pos;
        if (agg_nulls && agg_nulls[a]) {
          /* NullableSingleInputAggregationFunction.forEachNotNull (:118-160): the null docs of THIS column do not reach its holders */
          npos = 0;
          for (int32_t i = 0; i < pos; i++) {
            if ((agg_nulls[a][doc_ids[i] >> 6] >> (doc_ids[i] & 63)) & 1) continue;
            nn_gids[npos] = group_ids[i]; dbl_values[npos] = dbl_values[i]; vals.i[npos] = vals.i[i]; vals.l[npos] = vals.l[i];
            npos++;
          }
          gids = nn_gids;
        }
        for (int32_t i = 0; i < npos; i++) gnn[(size_t)a * G + gids[i]]++;
#define group_ids gids
#define pos npos
        if (func == PG_AGG_SUM || func == PG_AGG_AVG) {
          if (st == PG_TYPE_INT) for (int32_t i = 0; i < pos; i++) exact_add(&ex[group_ids[i]], vals.i[i], &gover[(size_t)a * G + group_ids[i]]);
          if (st == PG_TYPE_LONG) for (int32_t i = 0; i < pos; i++) exact_add(&ex[group_ids[i]], vals.l[i], &gover[(size_t)a * G + group_ids[i]]);
        }
        switch (func) {
          case PG_AGG_SUM: /* SumAggregationFunction.aggregateGroupBySV :173-178 */
            for (int32_t i = 0; i < pos; i++) hold[group_ids[i]] = hold[group_ids[i]] + dbl_values[i];
            break;
          case PG_AGG_MAX: /* MaxAggregationFunction.aggregateGroupBySV :180-187 */
            for (int32_t i = 0; i < pos; i++) if (dbl_values[i] > hold[group_ids[i]]) hold[group_ids[i]] = dbl_values[i];
            break;
          case PG_AGG_MIN:
            for (int32_t i = 0; i < pos; i++) if (dbl_values[i] < hold[group_ids[i]]) hold[group_ids[i]] = dbl_values[i];
            break;
          case PG_AGG_AVG:
            for (int32_t i = 0; i < pos; i++) { gavg_sum[(size_t)a * G + group_ids[i]] += dbl_values[i]; gavg_cnt[(size_t)a * G + group_ids[i]] += 1; }
            break;
          default: rc = 2; snprintf(po_error, sizeof(po_error), "unsupported aggregation %d", func); goto cleanup;
        }
#undef group_ids
#undef pos
      }
    }
  }

  /* results */
  res->num_aggregations = na;
  if (ng == 0) {
    res->aggregations = (pg_agg_value*)calloc((size_t)(na > 0 ? na : 1), sizeof(pg_agg_value));
    for (int a = 0; a < na; a++) {
      pg_agg_value* v = &res->aggregations[a];
      int func = q->aggregations[a].function;
      v->min = INFINITY; v->max = -INFINITY;
      v->count = func == PG_AGG_COUNT ? (int64_t)holders[a].value : (func == PG_AGG_AVG ? holders[a].avg_count : holders[a].n);
      const int integral = func != PG_AGG_COUNT && seg->columns[q->aggregations[a].column].stored_type <= PG_TYPE_LONG && !holders[a].overflow;
      if (func == PG_AGG_SUM) { v->sum = holders[a].value; v->sum_i64 = holders[a].exact_sum; v->sum_exact = integral; }
      if (func == PG_AGG_AVG) { v->sum = holders[a].avg_sum; v->sum_i64 = holders[a].exact_sum; v->sum_exact = integral; }
      if (func == PG_AGG_MIN) v->min = holders[a].value;
      if (func == PG_AGG_MAX) v->max = holders[a].value;
    }
  } else {
    size_t G = (size_t)group_upper;
    int32_t num_groups = 0;
    for (size_t g = 0; g < G; g++) num_groups += flags[g];
    res->num_groups = num_groups;
    res->group_id_upper_bound = (int32_t)group_upper;
    res->group_ids = (int32_t*)malloc(sizeof(int32_t) * (size_t)(num_groups > 0 ? num_groups : 1));
    res->group_key_kind = key_kind;
    res->group_key_dict_ids = (int32_t*)malloc(sizeof(int32_t) * (size_t)(num_groups > 0 ? num_groups : 1) * (size_t)(ng > 0 ? ng : 1));
    if (key_kind == 1) res->group_ids64 = (int64_t*)malloc(sizeof(int64_t) * (size_t)(num_groups > 0 ? num_groups : 1));
    res->group_aggregations = (pg_agg_value*)calloc((size_t)(num_groups > 0 ? num_groups : 1) * (size_t)(na > 0 ? na : 1), sizeof(pg_agg_value));
    int32_t k = 0;
    /* result rows in ascending raw-key order (the ABI's order; the reference's own iteration order is the hash map's) */
    int32_t* order = NULL;
    if (map_based) {
      order = (int32_t*)malloc(sizeof(int32_t) * (size_t)(map_size > 0 ? map_size : 1));
      for (int32_t i = 0; i < map_size; i++) order[i] = i;
      po_sort_keys = raw_of_gid; po_sort_ng = ng;
      qsort(order, (size_t)map_size, sizeof(int32_t), po_cmp_by_key);
      res->num_groups_limit_reached = map_size >= num_groups_limit;      /* GroupByOperator.java:114-115 */
    }
    for (size_t idx = 0; idx < (map_based ? (size_t)map_size : G); idx++) {
      const size_t g = map_based ? (size_t)order[idx] : idx;
      if (!flags[g]) continue;
      {
        /* the key as the ABI returns it: int raw key / long raw key / row number, and always the dictId tuple */
        po_key key;
        if (map_based) key = raw_of_gid[g];
        else { uint64_t raw = (uint64_t)g; for (int c = 0; c < ng; c++) { key.d[c] = (int32_t)(raw % (uint64_t)cards[c]); raw /= (uint64_t)cards[c]; } }
        res->group_ids[k] = key_kind == 0 ? (int32_t)po_key_value(&key, cards, ng) : k;
        if (key_kind == 1) res->group_ids64[k] = (int64_t)po_key_value(&key, cards, ng);
        for (int c = 0; c < ng; c++) res->group_key_dict_ids[(size_t)k * (size_t)ng + (size_t)c] = key.d[c];
      }
      for (int a = 0; a < na; a++) {
        pg_agg_value* v = &res->group_aggregations[(size_t)k * (size_t)na + (size_t)a];
        int func = q->aggregations[a].function;
        v->min = INFINITY; v->max = -INFINITY;
        v->count = func == PG_AGG_COUNT ? (int64_t)gholders[(size_t)a * G + g] : (func == PG_AGG_AVG ? gavg_cnt[(size_t)a * G + g] : gnn[(size_t)a * G + g]);
        const int integral = func != PG_AGG_COUNT && seg->columns[q->aggregations[a].column].stored_type <= PG_TYPE_LONG && !gover[(size_t)a * G + g];
        if (func == PG_AGG_SUM) { v->sum = gholders[(size_t)a * G + g]; v->sum_i64 = gexact[(size_t)a * G + g]; v->sum_exact = integral; }
        if (func == PG_AGG_AVG) { v->sum = gavg_sum[(size_t)a * G + g]; v->sum_i64 = gexact[(size_t)a * G + g]; v->sum_exact = integral; }
        if (func == PG_AGG_MIN) v->min = gholders[(size_t)a * G + g];
        if (func == PG_AGG_MAX) v->max = gholders[(size_t)a * G + g];
      }
      k++;
    }
    free(order);
    res->group_id_upper_bound = (key_kind == 0 && !no_dict_keys) ? (int32_t)raw_key_upper : num_groups_limit;      /* LongMap / ArrayMap / no-dictionary generators: _globalGroupIdUpperBound = numGroupsLimit (:150-163) */
  }
  /* ExecutionStatistics: AggregationOperator.java:88-93 (numDocsScanned, inFilter, numDocsScanned * numProjectedColumns, totalDocs) */
  {
    int proj[64]; int nproj = 0;
    for (int g = 0; g < ng; g++) { int c = q->group_by_columns[g], seen = 0; for (int j = 0; j < nproj; j++) seen |= proj[j] == c; if (!seen && nproj < 64) proj[nproj++] = c; }
    for (int a = 0; a < na; a++) { int c = q->aggregations[a].column; if (c < 0) continue; int seen = 0; for (int j = 0; j < nproj; j++) seen |= proj[j] == c; if (!seen && nproj < 64) proj[nproj++] = c; }
    if (it->kind == 1) entries_in_filter = it->scan.num_entries_scanned;
    res->stats.num_docs_scanned = num_docs_scanned;
    res->stats.num_entries_scanned_in_filter = entries_in_filter;
    res->filter_entries_exact = null_handling ? 0 : 1;     /* the iterator accounting above; under enableNullHandling: full scans per leaf */
    res->stats.num_entries_scanned_post_filter = num_docs_scanned * nproj;
    res->stats.num_total_docs = num_docs;
  }

cleanup:
  free(doc_ids); free(dict_scratch); free(vals.i); free(vals.l); free(vals.f); free(vals.d); free(dbl_values); free(group_ids); free(raw_keys); free(nn_gids); free(gnn);
  for (int g = 0; g < PO_MAX_GROUP_COLS; g++) free(key_nulls[g]);
  free(holders); free(gholders); free(gavg_sum); free(gavg_cnt); free(gexact); free(gover); free(gcount); free(flags);
  free(map_keys); free(map_used); free(map_ids); free(raw_of_gid);
done:
  for (int g = 0; g < PO_MAX_GROUP_COLS; g++) free(rank_dict[g]);
  if (agg_nulls) for (int a = 0; a < q->num_aggregations; a++) free(agg_nulls[a]);
  free(agg_nulls);
  free(filter_words); free(it); free(cols);
  return rc;
}

void po_result_free(pg_result* res) {
  if (!res) return;
  free(res->aggregations); free(res->group_ids); free(res->group_ids64); free(res->group_key_dict_ids); free(res->group_aggregations);
  memset(res, 0, sizeof(*res));
}

/* Filter only -> dense bitmap (used to check pg_filter_bitmap). */
int po_filter_bitmap(const pg_segment_desc* seg, const pg_query* q, uint64_t* out_words, int64_t num_words, int64_t* out_cardinality) {
  po_column* cols = (po_column*)calloc((size_t)(seg->num_columns > 0 ? seg->num_columns : 1), sizeof(po_column));
  for (int32_t c = 0; c < seg->num_columns; c++) {
    cols[c].desc = &seg->columns[c];
    if (seg->columns[c].fwd_encoding == PG_FWD_RAW_FIXED_BYTE &&
        po_raw_open((const uint8_t*)seg->columns[c].fwd_data, seg->columns[c].fwd_size, &cols[c].raw)) { free(cols); return 1; }
  }
  uint64_t* words = NULL; int64_t entries = 0;
  int rc = filter_to_bitmap(cols, seg, q, &words, &entries);
  free(cols);
  if (rc) return rc;
  int64_t nw = bitmap_words(seg->num_docs);
  if (num_words < nw) { free(words); PO_FAIL(1, "bitmap buffer too small"); }
  int64_t card = 0;
  for (int64_t i = 0; i < nw; i++) { out_words[i] = words[i]; card += __builtin_popcountll(words[i]); }
  if (out_cardinality) *out_cardinality = card;
  free(words);
  return 0;
}

/* BlockValSet.getDoubleValuesSV on any numeric stored type (and getLongValuesSV for INT / LONG). */
int po_read_double_values(const pg_segment_desc* seg, int32_t column, const int32_t* doc_ids, int32_t length, double* out, int64_t* out_long) {
  po_column col; memset(&col, 0, sizeof(col));
  col.desc = &seg->columns[column];
  if (col.desc->fwd_encoding == PG_FWD_RAW_FIXED_BYTE && po_raw_open((const uint8_t*)col.desc->fwd_data, col.desc->fwd_size, &col.raw)) return 1;
  size_t n = (size_t)(length > 0 ? length : 1);
  int32_t* scratch = (int32_t*)malloc(sizeof(int32_t) * n);
  po_values v;
  v.i = (int32_t*)malloc(4 * n); v.l = (int64_t*)malloc(8 * n); v.f = (float*)malloc(4 * n); v.d = (double*)malloc(8 * n);
  fetch_stored_values(&col, seg->num_docs, doc_ids, length, scratch, &v);
  widen_to_double(col.desc->stored_type, &v, length, out);
  if (out_long) {
    if (col.desc->stored_type == PG_TYPE_INT) for (int32_t i = 0; i < length; i++) out_long[i] = v.i[i];
    else if (col.desc->stored_type == PG_TYPE_LONG) for (int32_t i = 0; i < length; i++) out_long[i] = v.l[i];
    else for (int32_t i = 0; i < length; i++) out_long[i] = (int64_t)out[i];
  }
  free(scratch); free(v.i); free(v.l); free(v.f); free(v.d);
  return 0;
}

/* BlockValSet-level readers for SPI parity tests. */
int po_read_int_values(const pg_segment_desc* seg, int32_t column, const int32_t* doc_ids, int32_t length, int32_t* out) {
  po_column col; memset(&col, 0, sizeof(col));
  col.desc = &seg->columns[column];
  if (col.desc->stored_type != PG_TYPE_INT) PO_FAIL(2, "po_read_int_values: column is not INT");
  if (col.desc->fwd_encoding == PG_FWD_RAW_FIXED_BYTE && po_raw_open((const uint8_t*)col.desc->fwd_data, col.desc->fwd_size, &col.raw)) return 1;
  int32_t* scratch = (int32_t*)malloc(sizeof(int32_t) * (size_t)(length > 0 ? length : 1));
  fetch_int_values(&col, seg->num_docs, doc_ids, length, scratch, out);
  free(scratch);
  return 0;
}
