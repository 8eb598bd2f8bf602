// c_api.cpp -- flat C facade over the C++ host mirror so that Python tests can drive
// GpuPlanMaker.makeSegmentPlanNode(...).run().nextBlock() and the combine step the way the reference's
// BaseQueriesTest.getOperator(sql) / getBrokerResponse(sql, planMaker) do (BaseQueriesTest.java:100-105,154-156).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>

#include "pinot_host.h"
#include "../pg_raw_set_table.h"
#include "../pg_hll.h"
#include "../pg_chunk_codec.h"

using namespace pinot;

namespace {
thread_local std::string g_hostError;
GpuPlanMaker g_planMaker;

std::string jsonEscape(const std::string& s) {
  std::string o;
  for (char c : s) {
    if (c == '"' || c == '\\') { o += '\\'; o += c; }
    else if ((unsigned char)c < 0x20) { char b[8]; snprintf(b, sizeof(b), "\\u%04x", c); o += b; }
    else o += c;
  }
  return o;
}

std::string num(double v) {
  if (std::isinf(v)) return v > 0 ? "\"Infinity\"" : "\"-Infinity\"";
  if (std::isnan(v)) return "\"NaN\"";        // bare nan is not JSON
  char b[64];
  snprintf(b, sizeof(b), "%.17g", v);
  return b;
}

std::string intermediateJson(const IntermediateResult& r) {
  if (isNullResult(r)) return "null";
  if (std::holds_alternative<int64_t>(r)) return std::to_string(std::get<int64_t>(r));
  if (std::holds_alternative<double>(r)) return num(std::get<double>(r));
  if (std::holds_alternative<ValueSet>(r)) {
    // the value set: INT / LONG values as they are, FLOAT / DOUBLE values from their bit images
    const ValueSet& s = std::get<ValueSet>(r);
    const bool floating = s.storedType == DataType::FLOAT || s.storedType == DataType::DOUBLE;
    std::string out = "{\"values\": [";
    for (size_t i = 0; i < s.values.size(); ++i) {
      if (i) out += ", ";
      if (floating) { double v; memcpy(&v, &s.values[i], 8); out += num(v); } else out += std::to_string(s.values[i]);
    }
    return out + "]}";
  }
  if (std::holds_alternative<HllRegisters>(r)) {
    // the sketch as its registers, one rank each
    const HllRegisters& h = std::get<HllRegisters>(r);
    std::string out = "{\"registers\": [";
    for (size_t i = 0; i < h.registers.size(); ++i) out += (i ? ", " : "") + std::to_string((int)h.registers[i]);
    return out + "]}";
  }
  if (std::holds_alternative<ValueCounts>(r)) {
    // the value list as its ascending runs
    const ValueCounts& l = std::get<ValueCounts>(r);
    std::string out = "{\"values\": [";
    for (size_t i = 0; i < l.values.size(); ++i) out += (i ? ", " : "") + num(l.values[i]);
    out += "], \"counts\": [";
    for (size_t i = 0; i < l.counts.size(); ++i) out += (i ? ", " : "") + std::to_string(l.counts[i]);
    return out + "]}";
  }
  if (std::holds_alternative<VarianceTuple>(r)) {
    const VarianceTuple& t = std::get<VarianceTuple>(r);
    return "{\"count\": " + std::to_string(t.count) + ", \"sum\": " + num(t.sum) + ", \"m2\": " + num(t.m2) + "}";
  }
  const AvgPair& p = std::get<AvgPair>(r);
  return "[" + num(p.sum) + ", " + std::to_string(p.count) + "]";
}

std::string blockJson(const ResultsBlock& b) {
  std::ostringstream o;
  o << "{\"isGroupBy\": " << (b.isGroupBy ? "true" : "false");
  const auto& functions = b.isGroupBy ? b.groupBy.functions : b.aggregation.functions;
  o << ", \"columns\": [";
  for (size_t i = 0; i < functions.size(); ++i) o << (i ? ", " : "") << "\"" << jsonEscape(functions[i].getResultColumnName()) << "\"";
  o << "]";
  if (!b.isGroupBy) {
    o << ", \"intermediate\": [";
    for (size_t i = 0; i < functions.size(); ++i) o << (i ? ", " : "") << intermediateJson(b.aggregation.results[i]);
    o << "], \"final\": [";
    for (size_t i = 0; i < functions.size(); ++i)
      o << (i ? ", " : "") << (isNullResult(b.aggregation.results[i]) ? std::string("null") : num(functions[i].extractFinalResult(b.aggregation.results[i])));
    o << "]";
  } else {
    o << ", \"groupByColumns\": [";
    for (size_t i = 0; i < b.groupBy.groupByColumns.size(); ++i) o << (i ? ", " : "") << "\"" << jsonEscape(b.groupBy.groupByColumns[i]) << "\"";
    o << "], \"groups\": [";
    for (size_t g = 0; g < b.groupBy.groupKeys.size(); ++g) {
      o << (g ? ", " : "") << "{\"key\": [";
      const auto& keys = b.groupBy.groupKeys[g].keys;
      for (size_t k = 0; k < keys.size(); ++k) {
        o << (k ? ", " : "");
        if (std::holds_alternative<std::monostate>(keys[k])) o << "null";
        else if (std::holds_alternative<int64_t>(keys[k])) o << std::get<int64_t>(keys[k]);
        else if (std::holds_alternative<double>(keys[k])) o << num(std::get<double>(keys[k]));
        else o << "\"" << jsonEscape(std::get<std::string>(keys[k])) << "\"";
      }
      o << "], \"intermediate\": [";
      for (size_t i = 0; i < functions.size(); ++i) o << (i ? ", " : "") << intermediateJson(b.groupBy.results[g][i]);
      o << "], \"final\": [";
      for (size_t i = 0; i < functions.size(); ++i)
        o << (i ? ", " : "") << (isNullResult(b.groupBy.results[g][i]) ? std::string("null") : num(functions[i].extractFinalResult(b.groupBy.results[g][i])));
      o << "]}";
    }
    o << "]";
  }
  o << ", \"stats\": {\"numDocsScanned\": " << b.stats.numDocsScanned << ", \"numEntriesScannedInFilter\": " << b.stats.numEntriesScannedInFilter
    << ", \"numEntriesScannedPostFilter\": " << b.stats.numEntriesScannedPostFilter << ", \"numTotalDocs\": " << b.stats.numTotalDocs << "}";
  if (b.isGroupBy) o << ", \"numGroupsLimitReached\": " << (b.numGroupsLimitReached ? "true" : "false");
  o << ", \"deviceMs\": " << num(b.deviceMs) << ", \"kernelMs\": " << num(b.kernelMs) << "}";
  return o.str();
}

// the broker's rows (GroupByDataTableReducer): [[key..., final...], ...] in ORDER BY order, at most LIMIT of them
std::string reducedJson(const std::vector<ReducedRow>& rows) {
  std::ostringstream o;
  o << "[";
  for (size_t r = 0; r < rows.size(); ++r) {
    o << (r ? ", " : "") << "[";
    bool first = true;
    for (const auto& k : rows[r].keys) {
      o << (first ? "" : ", ");
      first = false;
      if (std::holds_alternative<std::monostate>(k)) o << "null";
      else if (std::holds_alternative<int64_t>(k)) o << std::get<int64_t>(k);
      else if (std::holds_alternative<double>(k)) o << num(std::get<double>(k));
      else o << "\"" << jsonEscape(std::get<std::string>(k)) << "\"";
    }
    for (const auto& v : rows[r].finals) {
      o << (first ? "" : ", ");
      first = false;
      if (std::holds_alternative<std::monostate>(v)) o << "null";
      else if (std::holds_alternative<int64_t>(v)) o << std::get<int64_t>(v);
      else if (std::holds_alternative<double>(v)) o << num(std::get<double>(v));
      else o << "\"" << jsonEscape(std::get<std::string>(v)) << "\"";
    }
    o << "]";
  }
  o << "]";
  return o.str();
}

// A results block from flat arrays (ph_datatable_v4_build / ph_group_by_combine: tests drive the writers and the combine without a
// device): rows [row_begin, row_end) of the arrays.
ResultsBlock blockFromArrays(bool is_group_by, const std::vector<AggregationFunction>& functions, int32_t num_keys, const char* const* key_names,
                             const int32_t* key_types, int64_t row_begin, int64_t row_end, const int64_t* key_longs, const double* key_doubles,
                             const char* const* key_strings, const uint8_t* key_is_null, const int64_t* counts, const double* sums, const double* mins,
                             const double* maxs, const uint8_t* is_null, const int64_t* set_offsets = nullptr, const int64_t* set_values = nullptr,
                             const int64_t* run_offsets = nullptr, const double* run_values = nullptr, const int64_t* run_counts = nullptr,
                             const int64_t* register_offsets = nullptr, const uint8_t* registers = nullptr, const double* m2s = nullptr) {
  ResultsBlock block;
  block.isGroupBy = is_group_by;
  const int num_functions = (int)functions.size();
  auto value = [&](int64_t row, int f) -> IntermediateResult {
    const size_t at = (size_t)row * (size_t)num_functions + (size_t)f;
    if (is_null && is_null[at]) return std::monostate{};
    switch (functions[(size_t)f].getType()) {
      case AggregationFunctionType::DISTINCTCOUNT: {
        // cell `at` holds the LONG values set_values[set_offsets[at] .. set_offsets[at + 1]) (any order, duplicates allowed)
        ValueSet s;
        s.storedType = DataType::LONG;
        if (set_offsets && set_values) s.values.assign(set_values + set_offsets[at], set_values + set_offsets[at + 1]);
        std::sort(s.values.begin(), s.values.end());
        s.values.erase(std::unique(s.values.begin(), s.values.end()), s.values.end());
        return s;
      }
      case AggregationFunctionType::DISTINCTCOUNTHLL: {
        // cell `at` holds the registers registers[register_offsets[at] .. register_offsets[at + 1]): 2^log2m bytes, or none (an empty sketch of the function's log2m)
        if (!register_offsets || !registers || register_offsets[at + 1] == register_offsets[at]) return HllRegisters::empty(functions[(size_t)f].getHllLog2m());
        return HllRegisters::fromDeviceRegisters(registers + register_offsets[at], (int32_t)(register_offsets[at + 1] - register_offsets[at]));
      }
      case AggregationFunctionType::PERCENTILE: {
        // cell `at` holds the runs (run_values[i], run_counts[i]), i in [run_offsets[at], run_offsets[at + 1]): any order, values may repeat
        ValueCounts l;
        if (run_offsets && run_values && run_counts) {
          std::vector<std::pair<double, int64_t>> runs;
          for (int64_t i = run_offsets[at]; i < run_offsets[at + 1]; ++i) if (run_counts[i] > 0) runs.emplace_back(run_values[i], run_counts[i]);
          // (NaN last, as Double.compare has it: operator< alone is no ordering once a NaN is among the values)
          std::sort(runs.begin(), runs.end(), [](const std::pair<double, int64_t>& p, const std::pair<double, int64_t>& q) {
            const bool pn = p.first != p.first, qn = q.first != q.first;
            return (pn || qn) ? (!pn && qn) : p < q;
          });
          for (const auto& run : runs) {
            if (!l.values.empty() && (l.values.back() == run.first || (l.values.back() != l.values.back() && run.first != run.first))) l.counts.back() += run.second;
            else { l.values.push_back(run.first); l.counts.push_back(run.second); }
          }
        }
        return l;
      }
      // cell `at` of a variance function holds the VarianceTuple (counts[at], sums[at], m2s[at])
      case AggregationFunctionType::VARPOP: case AggregationFunctionType::VARSAMP: case AggregationFunctionType::STDDEVPOP: case AggregationFunctionType::STDDEVSAMP:
        return VarianceTuple{counts[at], sums[at], m2s ? m2s[at] : 0.0};
      case AggregationFunctionType::COUNT: return counts[at];
      case AggregationFunctionType::SUM: return sums[at];
      case AggregationFunctionType::MIN: return mins[at];
      case AggregationFunctionType::MAX: return maxs[at];
      default: return AvgPair{sums[at], counts[at]};
    }
  };
  if (!block.isGroupBy) {
    block.aggregation.functions = functions;
    for (int f = 0; f < num_functions; ++f) block.aggregation.results.push_back(value(row_begin, f));
    return block;
  }
  GroupByResultsBlock& g = block.groupBy;
  g.functions = functions;
  for (int k = 0; k < num_keys; ++k) { g.groupByColumns.push_back(key_names[k]); g.groupByTypes.push_back((DataType)key_types[k]); }
  for (int64_t r = row_begin; r < row_end; ++r) {
    GroupKey key;
    key.groupId = (int)(r - row_begin);
    for (int k = 0; k < num_keys; ++k) {
      const size_t at = (size_t)r * (size_t)num_keys + (size_t)k;
      const DataType t = (DataType)key_types[k];
      if (key_is_null && key_is_null[at]) key.keys.emplace_back(std::monostate{});
      else if (t == DataType::INT || t == DataType::LONG) key.keys.emplace_back(key_longs[at]);
      else if (t == DataType::STRING) key.keys.emplace_back(std::string(key_strings[at]));
      else key.keys.emplace_back(key_doubles[at]);
    }
    g.groupKeys.push_back(std::move(key));
    std::vector<IntermediateResult> row;
    for (int f = 0; f < num_functions; ++f) row.push_back(value(r, f));
    g.results.push_back(std::move(row));
  }
  return block;
}

std::string resultTableJson(const ResultTable& t) {
  std::ostringstream o;
  o << "{\"columns\": [";
  for (size_t i = 0; i < t.columnNames.size(); ++i) o << (i ? ", " : "") << "\"" << jsonEscape(t.columnNames[i]) << "\"";
  o << "], \"rows\": [";
  for (size_t r = 0; r < t.rows.size(); ++r) {
    o << (r ? ", " : "") << "[";
    for (size_t i = 0; i < t.rows[r].size(); ++i) {
      const OrderByValue& v = t.rows[r][i];
      o << (i ? ", " : "");
      if (std::holds_alternative<std::monostate>(v)) o << "null";
      else if (std::holds_alternative<int64_t>(v)) o << std::get<int64_t>(v);
      else if (std::holds_alternative<double>(v)) o << num(std::get<double>(v));
      else o << "\"" << jsonEscape(std::get<std::string>(v)) << "\"";
    }
    o << "]";
  }
  o << "]}";
  return o.str();
}

template <typename F>
int guarded(F f) {
  try { f(); return 0; }
  catch (const QueryException& e) { g_hostError = e.what(); return 1; }
  catch (const UnsupportedOperationException& e) { g_hostError = e.what(); return 2; }
  catch (const std::exception& e) { g_hostError = e.what(); return 3; }
}
}  // namespace

extern "C" {

const char* ph_last_error(void) { return g_hostError.c_str(); }
void ph_free(char* p) { free(p); }

// Attaches the null value vector file of a column added earlier (the buffer stays caller-owned like the other index buffers).
int32_t ph_segment_set_null_vector(void* seg, const char* column, const void* data, uint64_t size) {
  return guarded([&] {
    ImmutableSegment* s = static_cast<ImmutableSegment*>(seg);
    DataSource& ds = s->mutableDataSource(column ? column : "");
    ds.nullValueVector = (const uint8_t*)data;
    ds.nullValueVectorSize = size;
  });
}

// SegmentContext.getQueryableDocIdsSnapshot() of an upsert / dedup table's segment: one serialized RoaringBitmap of the valid docIds (copied);
// NULL clears it.  Every query over the segment then runs behind it (FilterPlanNode.java:88-106).
int32_t ph_segment_set_queryable_doc_ids(void* seg, const void* roaring_bytes, uint64_t size) {
  return guarded([&] { static_cast<ImmutableSegment*>(seg)->setQueryableDocIds(roaring_bytes, size); });
}

// Segments assembled column by column have no metadata.properties: isSorted is derived from the data the way the segment creator's
// column statistics do (a dictionary column whose dictIds never decrease in docId order, AbstractColumnStatisticsCollector), together
// with the [start, end] docId pair of every dictId that SortedIndexReaderImpl would hold.  Unsorted columns leave at the first descent.
static void detectSorted(DataSource* ds, int numDocs) {
  if (!ds->hasDictionary || ds->forwardIndex == nullptr || ds->bitsPerElement <= 0 || ds->bitsPerElement > 31 || numDocs <= 0 || ds->cardinality <= 0) return;
  const int b = ds->bitsPerElement;
  if (ds->forwardIndexSize < ((uint64_t)numDocs * (uint64_t)b + 7) / 8) return;
  std::vector<int32_t> ranges((size_t)ds->cardinality * 2, -1);
  int32_t previous = -1;
  for (int64_t doc = 0; doc < numDocs; ++doc) {
    const uint64_t bit = (uint64_t)doc * (uint64_t)b;
    uint64_t window = 0;                                      // the 5 bytes that hold the value, MSB first (PinotDataBitSet layout)
    for (int k = 0; k < 5; ++k) { const uint64_t at = (bit >> 3) + (uint64_t)k; window = (window << 8) | (at < ds->forwardIndexSize ? ds->forwardIndex[at] : 0u); }
    const int32_t id = (int32_t)((window >> (40 - (int)(bit & 7) - b)) & ((1ull << b) - 1ull));
    if (id < previous || id >= ds->cardinality) return;
    if (id != previous) ranges[2 * (size_t)id] = (int32_t)doc;
    ranges[2 * (size_t)id + 1] = (int32_t)doc;
    previous = id;
  }
  for (int32_t r : ranges) if (r < 0) return;                 // a dictionary entry no doc uses: not a creator-built segment
  ds->isSorted = true;
  ds->sortedDocIdRanges = std::move(ranges);
}

void* ph_segment_create(const char* name, int32_t num_docs) { return new ImmutableSegment(name ? name : "", num_docs); }

int32_t ph_segment_add_int_column(void* seg, const char* name, int32_t has_dictionary, int32_t bits, int32_t cardinality, const void* fwd,
                                  uint64_t fwd_size, const void* dict, uint64_t dict_size, const void* inv, uint64_t inv_size) {
  return guarded([&] {
    DataSource ds;
    ds.name = name;
    ds.dataType = DataType::INT;
    ds.hasDictionary = has_dictionary != 0;
    ds.bitsPerElement = bits;
    ds.cardinality = cardinality;
    ds.forwardIndex = (const uint8_t*)fwd; ds.forwardIndexSize = fwd_size;
    ds.dictionaryBuffer = (const uint8_t*)dict; ds.dictionaryBufferSize = dict_size;
    if (ds.hasDictionary) ds.dictionary = std::make_shared<IntDictionary>((const uint8_t*)dict, cardinality);
    ds.hasInvertedIndex = inv != nullptr && inv_size > 0;
    ds.invertedIndex = (const uint8_t*)inv; ds.invertedIndexSize = inv_size;
    detectSorted(&ds, ((ImmutableSegment*)seg)->getTotalDocs());
    ((ImmutableSegment*)seg)->addDataSource(std::move(ds));
  });
}

// data_type: 0 INT, 1 LONG, 2 FLOAT, 3 DOUBLE (pg_data_type).  Dictionary columns pass the big-endian fixed-width dictionary
// buffer; raw columns the PASS_THROUGH chunk file.
int32_t ph_segment_add_numeric_column(void* seg, const char* name, int32_t data_type, int32_t has_dictionary, int32_t bits, int32_t cardinality,
                                      const void* fwd, uint64_t fwd_size, const void* dict, uint64_t dict_size, const void* inv, uint64_t inv_size) {
  return guarded([&] {
    if (data_type < 0 || data_type > 3) throw QueryException("unknown data type");
    static const DataType kTypes[] = {DataType::INT, DataType::LONG, DataType::FLOAT, DataType::DOUBLE};
    DataSource ds;
    ds.name = name;
    ds.dataType = kTypes[data_type];
    ds.hasDictionary = has_dictionary != 0;
    ds.bitsPerElement = bits;
    ds.cardinality = cardinality;
    ds.forwardIndex = (const uint8_t*)fwd; ds.forwardIndexSize = fwd_size;
    ds.dictionaryBuffer = (const uint8_t*)dict; ds.dictionaryBufferSize = dict_size;
    if (ds.hasDictionary) {
      const uint8_t* d = (const uint8_t*)dict;
      switch (ds.dataType) {
        case DataType::INT: ds.dictionary = std::make_shared<IntDictionary>(d, cardinality); break;
        case DataType::LONG: ds.dictionary = std::make_shared<LongDictionary>(d, cardinality); break;
        case DataType::FLOAT: ds.dictionary = std::make_shared<FloatDictionary>(d, cardinality); break;
        default: ds.dictionary = std::make_shared<DoubleDictionary>(d, cardinality); break;
      }
    }
    ds.hasInvertedIndex = inv != nullptr && inv_size > 0;
    ds.invertedIndex = (const uint8_t*)inv; ds.invertedIndexSize = inv_size;
    detectSorted(&ds, ((ImmutableSegment*)seg)->getTotalDocs());
    ((ImmutableSegment*)seg)->addDataSource(std::move(ds));
  });
}

// values: `cardinality` NUL-terminated strings back to back, sorted ascending.
int32_t ph_segment_add_string_column(void* seg, const char* name, int32_t bits, int32_t cardinality, const void* fwd, uint64_t fwd_size,
                                     const char* values, const void* inv, uint64_t inv_size) {
  return guarded([&] {
    std::vector<std::string> vals;
    const char* p = values;
    for (int i = 0; i < cardinality; ++i) { vals.emplace_back(p); p += vals.back().size() + 1; }
    DataSource ds;
    ds.name = name;
    ds.dataType = DataType::STRING;
    ds.hasDictionary = true;
    ds.bitsPerElement = bits;
    ds.cardinality = cardinality;
    ds.forwardIndex = (const uint8_t*)fwd; ds.forwardIndexSize = fwd_size;
    ds.dictionary = std::make_shared<StringDictionary>(std::move(vals));
    ds.hasInvertedIndex = inv != nullptr && inv_size > 0;
    ds.invertedIndex = (const uint8_t*)inv; ds.invertedIndexSize = inv_size;
    detectSorted(&ds, ((ImmutableSegment*)seg)->getTotalDocs());
    ((ImmutableSegment*)seg)->addDataSource(std::move(ds));
  });
}

// ImmutableSegmentLoader.load(indexDir): opens a v1 / v3 segment directory and makes it HBM resident.  NULL + status on error.
void* ph_segment_load_directory(const char* index_dir, int32_t device, int32_t* status) {
  ImmutableSegment* out = nullptr;
  *status = guarded([&] {
    std::vector<std::string> skipped;
    std::unique_ptr<ImmutableSegment> seg = loadSegmentDirectory(index_dir ? index_dir : "", &skipped);
    seg->notOffloaded = std::move(skipped);
    if (device >= 0) seg->load(device);      // device < 0: host-side open only (metadata, dictionaries, buffers)
    out = seg.release();
  });
  return out;
}

// JSON description of a segment of the host mirror (columns as DataSourceMetadata sees them).
char* ph_segment_describe(void* segment, int32_t* status) {
  std::string out;
  *status = guarded([&] {
    const ImmutableSegment* seg = (const ImmutableSegment*)segment;
    std::ostringstream o;
    o << "{\"name\": \"" << jsonEscape(seg->getSegmentName()) << "\", \"totalDocs\": " << seg->getTotalDocs() << ", \"columns\": [";
    bool first = true;
    for (const DataSource& ds : seg->getDataSources()) {
      o << (first ? "" : ", ") << "{\"name\": \"" << jsonEscape(ds.name) << "\", \"dataType\": \"" << dataTypeName(ds.dataType) << "\", \"hasDictionary\": "
        << (ds.hasDictionary ? "true" : "false") << ", \"cardinality\": " << ds.cardinality << ", \"bitsPerElement\": " << ds.bitsPerElement
        << ", \"hasInvertedIndex\": " << (ds.hasInvertedIndex ? "true" : "false") << ", \"isSorted\": " << (ds.isSorted ? "true" : "false")
        << ", \"hasNullValueVector\": " << (ds.nullValueVector && ds.nullValueVectorSize ? "true" : "false");
      if (ds.dictionary && ds.cardinality > 0)
        o << ", \"minValue\": \"" << jsonEscape(ds.dictionary->getStringValue(0)) << "\", \"maxValue\": \"" << jsonEscape(ds.dictionary->getStringValue(ds.cardinality - 1)) << "\"";
      o << "}";
      first = false;
    }
    o << "], \"notOffloaded\": [";
    for (size_t i = 0; i < seg->notOffloaded.size(); ++i) o << (i ? ", " : "") << "\"" << jsonEscape(seg->notOffloaded[i]) << "\"";
    o << "]}";
    out = o.str();
  });
  return *status == 0 ? strdup(out.c_str()) : nullptr;
}

int32_t ph_segment_load(void* seg, int32_t device) { return guarded([&] { ((ImmutableSegment*)seg)->load(device); }); }
void ph_segment_destroy(void* seg) { delete (ImmutableSegment*)seg; }

int32_t ph_plan_maker_init(int32_t device, int32_t time_kernels) {
  return guarded([&] {
    std::map<std::string, std::string> cfg;
    cfg[GpuPlanMaker::kConfigDevice] = std::to_string(device);
    cfg[GpuPlanMaker::kConfigTimeKernels] = time_kernels ? "true" : "false";
    const char* batch = getenv("PINOT_GPU_HOST_BATCH");          // tests: "0" = every segment operator runs its own pg_execute
    cfg[GpuPlanMaker::kConfigBatch] = (batch && batch[0] == '0') ? "false" : "true";
    const char* exact = getenv("PINOT_GPU_HOST_EXACT_FILTER_STATS");      // tests: "0" = gpu.exact.filter.stats=false
    cfg[GpuPlanMaker::kConfigExactFilterStats] = (exact && exact[0] == '0') ? "false" : "true";
    g_planMaker.init(cfg);
  });
}

// gpu.devices parsing and least-loaded placement (no device touched): "[d0, d1, ...]" for `text`, then the device each of the `count`
// segment sizes goes to when opened in order -- the logic GpuPlanMaker.java / GpuSegmentCache.java carry in Java.
char* ph_plan_maker_placement(const char* devices_text, const int64_t* segment_bytes, int32_t count, int32_t* status) {
  std::string out;
  *status = guarded([&] {
    GpuPlanMaker pm;      // (not initialised: no device, no pg_init -- only its placement book)
    try { pm.setDevices(GpuPlanMaker::parseDevices(devices_text ? devices_text : "")); } catch (const std::invalid_argument& e) { throw QueryException(e.what()); }
    std::ostringstream o;
    o << "{\"devices\": [";
    for (size_t i = 0; i < pm.devices().size(); ++i) o << (i ? ", " : "") << pm.devices()[i];
    o << "], \"placement\": [";
    for (int32_t s = 0; s < count; ++s) {
      if (segment_bytes[s] < 0) pm.releaseSegment((int)(-segment_bytes[s] >> 48), (-segment_bytes[s]) & ((1ll << 48) - 1));      // tests: -(device << 48 | bytes) releases
      o << (s ? ", " : "") << (segment_bytes[s] < 0 ? -1 : pm.placeSegment((long long)segment_bytes[s]));
    }
    o << "]}";
    out = o.str();
  });
  return *status == 0 ? strdup(out.c_str()) : nullptr;
}

// Parse only (no device): returns a JSON description of the QueryContext; used by the CPU-side tests.
char* ph_parse_sql(const char* sql, int32_t* status) {
  std::string out;
  *status = guarded([&] {
    const QueryContext q = getQueryContext(sql);
    std::ostringstream o;
    o << "{\"table\": \"" << jsonEscape(q.tableName) << "\", \"aggregations\": [";
    for (size_t i = 0; i < q.aggregations.size(); ++i)
      o << (i ? ", " : "") << "\"" << jsonEscape(AggregationFunction(q.aggregations[i]).getResultColumnName()
                                                + (q.aggregations[i].hasFilter ? " FILTER(WHERE " + q.aggregations[i].filterText + ")" : std::string())) << "\"";
    o << "], \"groupBy\": [";
    for (size_t i = 0; i < q.groupByExpressions.size(); ++i) o << (i ? ", " : "") << "\"" << jsonEscape(q.groupByExpressions[i]) << "\"";
    o << "], \"hasFilter\": " << (q.hasFilter ? "true" : "false");
    if (q.nullHandlingEnabled) o << ", \"nullHandling\": true";
    if (q.hasOrderBy()) {
      o << ", \"orderBy\": [";
      for (size_t i = 0; i < q.orderByExpressions.size(); ++i) {
        const OrderByExpressionContext& ob = q.orderByExpressions[i];
        const std::string text = ob.isAggregation ? AggregationFunction(q.aggregations[(size_t)ob.index]).getResultColumnName()
                                                  : q.groupByExpressions[(size_t)ob.index];
        o << (i ? ", " : "") << "{\"expression\": \"" << jsonEscape(text) << "\", \"asc\": " << (ob.isAsc ? "true" : "false") << ", \"nullsLast\": "
          << (ob.isNullsLast() ? "true" : "false") << "}";
      }
      o << "]";
    }
    if (!q.groupByExpressions.empty()) o << ", \"limit\": " << q.limit;      // (aggregation-only results are one row whatever the limit)
    o << "}";
    out = o.str();
  });
  return *status == 0 ? strdup(out.c_str()) : nullptr;
}

// Lower one predicate against a dictionary buffer (no device): "[alwaysTrue, alwaysFalse, exclusive, isRange, start, end, n]"
char* ph_lower_predicate(const char* sql_predicate, const void* dict, int32_t cardinality, int32_t* status) {
  std::string out;
  *status = guarded([&] {
    const QueryContext q = getQueryContext(std::string("SELECT COUNT(*) FROM t WHERE ") + sql_predicate);
    if (q.filter.type != FilterContext::Type::PREDICATE) throw QueryException("expected a single predicate");
    DataSource ds;
    ds.name = q.filter.predicate.column;
    ds.cardinality = cardinality;
    ds.dictionary = std::make_shared<IntDictionary>((const uint8_t*)dict, cardinality);
    const PredicateEvaluator ev = getPredicateEvaluator(q.filter.predicate, ds);
    std::ostringstream o;
    o << "{\"alwaysTrue\": " << (ev.alwaysTrue ? "true" : "false") << ", \"alwaysFalse\": " << (ev.alwaysFalse ? "true" : "false")
      << ", \"exclusive\": " << (ev.exclusive ? "true" : "false") << ", \"isRange\": " << (ev.isRange ? "true" : "false")
      << ", \"start\": " << ev.startDictId << ", \"end\": " << ev.endDictId << ", \"dictIds\": [";
    for (size_t i = 0; i < ev.matchingDictIds.size(); ++i) o << (i ? ", " : "") << ev.matchingDictIds[i];
    o << "]}";
    out = o.str();
  });
  return *status == 0 ? strdup(out.c_str()) : nullptr;
}

// The physical filter tree of `sql`'s WHERE clause over a segment (which need not be loaded on a device): see explainFilter
char* ph_explain_filter(void* segment, const char* sql, int32_t* status) {
  std::string out;
  *status = guarded([&] { out = explainFilter(*(const ImmutableSegment*)segment, getQueryContext(sql)); });
  return *status == 0 ? strdup(out.c_str()) : nullptr;
}

// A RangePredicate given by its bounds ("*" = unbounded) against an INT dictionary buffer: RangePredicateEvaluatorFactory.newDictionaryBasedEvaluator
// (the reference's RangeOfflineDictionaryPredicateEvaluatorTest builds its predicates this way; SQL can only say one side at a time)
char* ph_lower_range_predicate(const void* dict, int32_t cardinality, const char* lower, int32_t lower_inclusive, const char* upper, int32_t upper_inclusive, int32_t* status) {
  std::string out;
  *status = guarded([&] {
    Predicate p;
    p.column = "column";
    p.type = Predicate::Type::RANGE;
    p.lowerBound = lower; p.lowerInclusive = lower_inclusive != 0;
    p.upperBound = upper; p.upperInclusive = upper_inclusive != 0;
    DataSource ds;
    ds.name = p.column;
    ds.cardinality = cardinality;
    ds.dictionary = std::make_shared<IntDictionary>((const uint8_t*)dict, cardinality);
    const PredicateEvaluator ev = getPredicateEvaluator(p, ds);
    std::ostringstream o;
    o << "{\"alwaysTrue\": " << (ev.alwaysTrue ? "true" : "false") << ", \"alwaysFalse\": " << (ev.alwaysFalse ? "true" : "false")
      << ", \"isRange\": " << (ev.isRange ? "true" : "false") << ", \"start\": " << ev.startDictId << ", \"end\": " << ev.endDictId
      << ", \"numMatchingItems\": " << ev.getNumMatchingItems() << "}";
    out = o.str();
  });
  return *status == 0 ? strdup(out.c_str()) : nullptr;
}

// A RangePredicate on a RAW (no-dictionary) INT (data_type 0), LONG (1), FLOAT (2) or DOUBLE (3) column:
// RangePredicateEvaluatorFactory.newRawValueBasedEvaluator; the evaluator matches lower <= value <= upper (both inclusive after the exclusive
// bounds were stepped inwards).  FLOAT / DOUBLE: rawLower / rawUpper are the bit patterns of the double bounds (as the ABI carries them),
// "lower" / "upper" the same bounds printed with %.17g.
char* ph_lower_raw_range_predicate(int32_t data_type, const char* lower, int32_t lower_inclusive, const char* upper, int32_t upper_inclusive, int32_t* status) {
  std::string out;
  *status = guarded([&] {
    Predicate p;
    p.column = "column";
    p.type = Predicate::Type::RANGE;
    p.lowerBound = lower; p.lowerInclusive = lower_inclusive != 0;
    p.upperBound = upper; p.upperInclusive = upper_inclusive != 0;
    DataSource ds;
    ds.name = p.column;
    ds.hasDictionary = false;
    static const DataType types[] = {DataType::INT, DataType::LONG, DataType::FLOAT, DataType::DOUBLE};
    if (data_type < 0 || data_type > 3) throw QueryException("raw range predicates take data types 0..3 (INT, LONG, FLOAT, DOUBLE)");
    ds.dataType = types[data_type];
    const PredicateEvaluator ev = getPredicateEvaluator(p, ds);
    std::ostringstream o;
    o << "{\"alwaysTrue\": " << (ev.alwaysTrue ? "true" : "false") << ", \"alwaysFalse\": " << (ev.alwaysFalse ? "true" : "false")
      << ", \"rawLower\": " << ev.rawLower << ", \"rawUpper\": " << ev.rawUpper;
    if (ev.rawFloating) {
      double lo, hi;
      char buf[64];
      memcpy(&lo, &ev.rawLower, 8); memcpy(&hi, &ev.rawUpper, 8);
      snprintf(buf, sizeof(buf), "%.17g", lo); o << ", \"lower\": \"" << buf << "\"";
      snprintf(buf, sizeof(buf), "%.17g", hi); o << ", \"upper\": \"" << buf << "\"";
    }
    o << "}";
    out = o.str();
  });
  return *status == 0 ? strdup(out.c_str()) : nullptr;
}

// The membership table of a PG_PRED_RAW_SET leaf (../pg_raw_set_table.h: what the engine builds and the kernels probe in LDS), built from
// `members` (bit patterns of 4- or 8-byte keys, distinct) and probed with the kernels' own lookup: out_hits[i] = 1 when probes[i] is found.
// Returns the table's bucket count, 0 when no table could be built.
int32_t ph_raw_set_table_probe(int32_t key_bytes, const uint64_t* members, int32_t num_members, const uint64_t* probes, int64_t num_probes, uint8_t* out_hits) {
  std::vector<uint64_t> keys(members, members + std::max(num_members, 0));
  pg::RawSetTable t;
  if (!pg::build_raw_set_table(keys, key_bytes, &t)) return 0;
  for (int64_t i = 0; i < num_probes; ++i) out_hits[i] = pg::raw_set_table_contains(t, probes[i]) ? 1 : 0;
  return (int32_t)t.buckets;
}

// getOperator(sql).nextBlock() per segment + the combined block: {"segments": [...], "combined": {...}}
char* ph_execute_sql(void** segments, int32_t num_segments, const char* sql, int32_t max_execution_threads, int32_t* status) {
  std::string out;
  *status = guarded([&] {
    const QueryContext q = getQueryContext(sql);
    std::vector<SegmentContext> ctxs;
    for (int i = 0; i < num_segments; ++i) ctxs.push_back(SegmentContext{(ImmutableSegment*)segments[i]});
    std::ostringstream o;
    o << "{\"segments\": [";
    for (int i = 0; i < num_segments; ++i) {
      auto op = g_planMaker.makeSegmentPlanNode(ctxs[(size_t)i], q)->run();
      const ResultsBlock b = op->nextBlock();
      o << (i ? ", " : "") << blockJson(b);
    }
    const ResultsBlock combined = g_planMaker.executeCombined(ctxs, q, max_execution_threads);
    o << "], \"combined\": " << blockJson(combined);
    if (combined.isGroupBy) {      // what the broker would answer: every key and final result ("reduced"), and the SELECT list's projection of it
      const std::vector<ReducedRow> rows = reduceGroupBy(combined, q);
      o << ", \"reduced\": " << reducedJson(rows) << ", \"resultTable\": " << resultTableJson(toResultTable(rows, combined, q));
    }
    o << "}";
    out = o.str();
  });
  return *status == 0 ? strdup(out.c_str()) : nullptr;
}

// DataTable V4 bytes of a results block given as flat arrays (tests drive the writer without a device through this):
// function_types: AggregationFunctionType ordinals (COUNT 0, SUM 1, MIN 2, MAX 3, AVG 4); key_types: DataType ordinals (INT 0, LONG 1,
// FLOAT 2, DOUBLE 3, STRING 4); per row and key the value comes from key_longs (INT / LONG), key_doubles (FLOAT / DOUBLE) or
// key_strings; per row and function: COUNT counts[], SUM sums[], MIN mins[], MAX maxs[], AVG (sums[], counts[]); is_null marks a null
// intermediate result (null handling).  stats: numDocsScanned, numEntriesScannedInFilter, numEntriesScannedPostFilter, numTotalDocs.
uint8_t* ph_datatable_v4_build(int32_t is_group_by, int32_t num_functions, const int32_t* function_types, const char* const* function_columns, int32_t num_keys,
                               const char* const* key_names, const int32_t* key_types, int64_t num_rows, const int64_t* key_longs, const double* key_doubles,
                               const char* const* key_strings, const int64_t* counts, const double* sums, const double* mins, const double* maxs,
                               const uint8_t* is_null, const int64_t* stats, int32_t null_handling, int32_t limit_reached, int32_t segments_processed,
                               int32_t segments_matched, int64_t* out_size, int32_t* status) {
  std::vector<uint8_t> bytes;
  *status = guarded([&] {
    std::vector<AggregationFunction> functions;
    for (int f = 0; f < num_functions; ++f) functions.emplace_back((AggregationFunctionType)function_types[f], function_columns[f], null_handling != 0);
    ResultsBlock block = blockFromArrays(is_group_by != 0, functions, num_keys, key_names, key_types, 0, num_rows, key_longs, key_doubles, key_strings, nullptr,
                                         counts, sums, mins, maxs, is_null);
    block.stats.numDocsScanned = stats[0]; block.stats.numEntriesScannedInFilter = stats[1];
    block.stats.numEntriesScannedPostFilter = stats[2]; block.stats.numTotalDocs = stats[3];
    block.numGroupsLimitReached = limit_reached != 0;
    bytes = toDataTableV4(block, null_handling != 0, segments_processed, segments_matched);
  });
  if (*status != 0) return nullptr;
  uint8_t* out = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);
  memcpy(out, bytes.data(), bytes.size());
  *out_size = (int64_t)bytes.size();
  return out;
}

// The DataTable V4 bytes the server would send for `sql` over these segments (combine, then InstanceResponseBlock.toDataTable().toBytes()).
// Returns a malloc-ed buffer (*out_size bytes, ph_free it) or NULL with *status set.
uint8_t* ph_execute_sql_datatable(void** segments, int32_t num_segments, const char* sql, int32_t max_execution_threads, int64_t* out_size, int32_t* status) {
  std::vector<uint8_t> bytes;
  *status = guarded([&] {
    const QueryContext q = getQueryContext(sql);
    std::vector<SegmentContext> ctxs;
    for (int i = 0; i < num_segments; ++i) ctxs.push_back(SegmentContext{(ImmutableSegment*)segments[i]});
    // numSegmentsMatched: segments with at least one doc scanned (BaseCombineOperator / InstanceResponseOperator bookkeeping)
    int matched = 0;
    for (int i = 0; i < num_segments; ++i) {
      const ResultsBlock b = g_planMaker.makeSegmentPlanNode(ctxs[(size_t)i], q)->run()->nextBlock();
      matched += b.stats.numDocsScanned > 0 ? 1 : 0;
    }
    bytes = toDataTableV4(g_planMaker.executeCombined(ctxs, q, max_execution_threads), q.nullHandlingEnabled, num_segments, matched);
  });
  if (*status != 0) return nullptr;
  uint8_t* out = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);
  memcpy(out, bytes.data(), bytes.size());
  *out_size = (int64_t)bytes.size();
  return out;
}

// GroupByCombineOperator + GroupByDataTableReducer over group-by blocks given as flat arrays (block b holds rows
// [sum(block_rows[0..b)), +block_rows[b]) of the arrays; same array conventions as ph_datatable_v4_build, key_is_null marks NULL keys).
// `sql` supplies the query context: aggregations (in the arrays' function order), GROUP BY columns, ORDER BY, LIMIT and the trim
// options.  Returns {"combined": <block>, "reduced": [[key..., final...], ...], "table": {resultSize, trimSize, trimThreshold, numResizes}}.
// ph_group_by_combine_sets: the same with the cells of DISTINCTCOUNT functions given as value sets -- cell (row, function) holds the LONG
// values set_values[set_offsets[row * functions + function] .. set_offsets[.. + 1]); the combine merges them by union.
char* ph_group_by_combine_sets(const char* sql, int32_t num_blocks, const int64_t* block_rows, const int32_t* key_types, const int64_t* key_longs,
                               const double* key_doubles, const char* const* key_strings, const uint8_t* key_is_null, const int64_t* counts, const double* sums,
                               const double* mins, const double* maxs, const uint8_t* is_null, const int64_t* set_offsets, const int64_t* set_values, int32_t* status);
char* ph_group_by_combine(const char* sql, int32_t num_blocks, const int64_t* block_rows, const int32_t* key_types, const int64_t* key_longs,
                          const double* key_doubles, const char* const* key_strings, const uint8_t* key_is_null, const int64_t* counts, const double* sums,
                          const double* mins, const double* maxs, const uint8_t* is_null, int32_t* status) {
  return ph_group_by_combine_sets(sql, num_blocks, block_rows, key_types, key_longs, key_doubles, key_strings, key_is_null, counts, sums, mins, maxs, is_null, nullptr, nullptr, status);
}
char* ph_group_by_combine_sets(const char* sql, int32_t num_blocks, const int64_t* block_rows, const int32_t* key_types, const int64_t* key_longs,
                               const double* key_doubles, const char* const* key_strings, const uint8_t* key_is_null, const int64_t* counts, const double* sums,
                               const double* mins, const double* maxs, const uint8_t* is_null, const int64_t* set_offsets, const int64_t* set_values, int32_t* status) {
  std::string out;
  *status = guarded([&] {
    const QueryContext q = getQueryContext(sql);
    if (q.groupByExpressions.empty()) throw QueryException("ph_group_by_combine needs a GROUP BY query");
    std::vector<AggregationFunction> functions;
    for (const auto& a : q.aggregations) functions.emplace_back(a, q.nullHandlingEnabled);
    std::vector<const char*> key_names;
    for (const auto& g : q.groupByExpressions) key_names.push_back(g.c_str());
    std::vector<ResultsBlock> blocks;
    int64_t row = 0;
    for (int b = 0; b < num_blocks; ++b) {
      ResultsBlock block = blockFromArrays(true, functions, (int32_t)key_names.size(), key_names.data(), key_types, row, row + block_rows[b], key_longs, key_doubles,
                                           key_strings, key_is_null, counts, sums, mins, maxs, is_null, set_offsets, set_values);
      trimSegmentGroupByBlock(&block, q);          // the segment operator's own trim comes first (GroupByOperator.java:119-135)
      blocks.push_back(std::move(block));
      row += block_rows[b];
    }
    if (blocks.empty()) throw QueryException("no blocks");
    const IndexedTable sizes = IndexedTable::forCombineOperator(functions, q);
    // count the resizes the way the combine operator's table does
    IndexedTable table = IndexedTable::forCombineOperator(functions, q);
    for (const auto& b : blocks) for (size_t i = 0; i < b.groupBy.groupKeys.size(); ++i) table.upsert(Record{b.groupBy.groupKeys[i].keys, b.groupBy.results[i]});
    table.finish(false);
    const ResultsBlock combined = combineGroupByBlocks(blocks, q);
    std::ostringstream o;
    const std::vector<ReducedRow> reduced = reduceGroupBy(combined, q);
    o << "{\"combined\": " << blockJson(combined) << ", \"reduced\": " << reducedJson(reduced) << ", \"resultTable\": " << resultTableJson(toResultTable(reduced, combined, q))
      << ", \"table\": {\"resultSize\": " << sizes.resultSize()
      << ", \"trimSize\": " << sizes.trimSize() << ", \"trimThreshold\": " << sizes.trimThreshold() << ", \"numResizes\": " << table.getNumResizes() << "}}";
    out = o.str();
  });
  return *status == 0 ? strdup(out.c_str()) : nullptr;
}

// The combine of PERCENTILE value lists built on the host (no device): one block per segment, the cells of PERCENTILE functions given as runs --
// cell (row, function) holds (run_values[i], run_counts[i]) for i in [run_offsets[row * functions + function], run_offsets[.. + 1]).  A GROUP BY
// query goes the way of ph_group_by_combine (same array conventions and result); an aggregation-only query has one row per block, is merged
// with AggregationResultsBlockMerger's mergeResultsBlocks and returns {"combined": <block>}.
char* ph_combine_counts(const char* sql, int32_t num_blocks, const int64_t* block_rows, const int32_t* key_types, const int64_t* key_longs,
                        const double* key_doubles, const char* const* key_strings, const uint8_t* key_is_null, const int64_t* counts, const double* sums,
                        const double* mins, const double* maxs, const uint8_t* is_null, const int64_t* run_offsets, const double* run_values,
                        const int64_t* run_counts, int32_t* status) {
  std::string out;
  *status = guarded([&] {
    const QueryContext q = getQueryContext(sql);
    std::vector<AggregationFunction> functions;
    for (const auto& a : q.aggregations) functions.emplace_back(a, q.nullHandlingEnabled);
    std::vector<const char*> key_names;
    for (const auto& g : q.groupByExpressions) key_names.push_back(g.c_str());
    const bool grouped = !q.groupByExpressions.empty();
    std::vector<ResultsBlock> blocks;
    int64_t row = 0;
    for (int b = 0; b < num_blocks; ++b) {
      if (!grouped && block_rows[b] != 1) throw QueryException("an aggregation-only block has one row");
      ResultsBlock block = blockFromArrays(grouped, functions, (int32_t)key_names.size(), key_names.data(), key_types, row, row + block_rows[b], key_longs, key_doubles,
                                           key_strings, key_is_null, counts, sums, mins, maxs, is_null, nullptr, nullptr, run_offsets, run_values, run_counts);
      if (grouped) trimSegmentGroupByBlock(&block, q);
      blocks.push_back(std::move(block));
      row += block_rows[b];
    }
    if (blocks.empty()) throw QueryException("no blocks");
    std::ostringstream o;
    if (!grouped) {
      ResultsBlock merged = blocks[0];
      for (size_t i = 1; i < blocks.size(); ++i) mergeResultsBlocks(&merged, blocks[i]);
      o << "{\"combined\": " << blockJson(merged) << "}";
    } else {
      const ResultsBlock combined = combineGroupByBlocks(blocks, q);
      const std::vector<ReducedRow> reduced = reduceGroupBy(combined, q);
      o << "{\"combined\": " << blockJson(combined) << ", \"reduced\": " << reducedJson(reduced) << ", \"resultTable\": " << resultTableJson(toResultTable(reduced, combined, q)) << "}";
    }
    out = o.str();
  });
  return *status == 0 ? strdup(out.c_str()) : nullptr;
}

// The combine of HyperLogLog registers built on the host (no device), the way ph_combine_counts drives PERCENTILE's: one block per segment, the cells of
// DISTINCTCOUNTHLL functions given as registers -- cell (row, function) holds the bytes registers[register_offsets[row * functions + function] ..
// register_offsets[.. + 1]) (2^log2m of them, or none for an empty sketch).  Same array conventions and results as ph_combine_counts.
char* ph_combine_hll(const char* sql, int32_t num_blocks, const int64_t* block_rows, const int32_t* key_types, const int64_t* key_longs,
                     const double* key_doubles, const char* const* key_strings, const uint8_t* key_is_null, const int64_t* counts, const double* sums,
                     const double* mins, const double* maxs, const uint8_t* is_null, const int64_t* register_offsets, const uint8_t* registers, int32_t* status) {
  std::string out;
  *status = guarded([&] {
    const QueryContext q = getQueryContext(sql);
    std::vector<AggregationFunction> functions;
    for (const auto& a : q.aggregations) functions.emplace_back(a, q.nullHandlingEnabled);
    std::vector<const char*> key_names;
    for (const auto& g : q.groupByExpressions) key_names.push_back(g.c_str());
    const bool grouped = !q.groupByExpressions.empty();
    std::vector<ResultsBlock> blocks;
    int64_t row = 0;
    for (int b = 0; b < num_blocks; ++b) {
      if (!grouped && block_rows[b] != 1) throw QueryException("an aggregation-only block has one row");
      ResultsBlock block = blockFromArrays(grouped, functions, (int32_t)key_names.size(), key_names.data(), key_types, row, row + block_rows[b], key_longs, key_doubles,
                                           key_strings, key_is_null, counts, sums, mins, maxs, is_null, nullptr, nullptr, nullptr, nullptr, nullptr, register_offsets, registers);
      if (grouped) trimSegmentGroupByBlock(&block, q);
      blocks.push_back(std::move(block));
      row += block_rows[b];
    }
    if (blocks.empty()) throw QueryException("no blocks");
    std::ostringstream o;
    if (!grouped) {
      ResultsBlock merged = blocks[0];
      for (size_t i = 1; i < blocks.size(); ++i) mergeResultsBlocks(&merged, blocks[i]);
      o << "{\"combined\": " << blockJson(merged) << "}";
    } else {
      const ResultsBlock combined = combineGroupByBlocks(blocks, q);
      const std::vector<ReducedRow> reduced = reduceGroupBy(combined, q);
      o << "{\"combined\": " << blockJson(combined) << ", \"reduced\": " << reducedJson(reduced) << ", \"resultTable\": " << resultTableJson(toResultTable(reduced, combined, q)) << "}";
    }
    out = o.str();
  });
  return *status == 0 ? strdup(out.c_str()) : nullptr;
}
// The combine of VarianceTuples built on the host (no device), the way ph_combine_hll drives the sketches': one block per segment, the cell of a
// VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP function carries (counts[at], sums[at], m2s[at]).  Same array conventions and results as ph_combine_counts.
char* ph_combine_moments(const char* sql, int32_t num_blocks, const int64_t* block_rows, const int32_t* key_types, const int64_t* key_longs,
                         const double* key_doubles, const char* const* key_strings, const uint8_t* key_is_null, const int64_t* counts, const double* sums,
                         const double* mins, const double* maxs, const uint8_t* is_null, const double* m2s, int32_t* status) {
  std::string out;
  *status = guarded([&] {
    const QueryContext q = getQueryContext(sql);
    std::vector<AggregationFunction> functions;
    for (const auto& a : q.aggregations) functions.emplace_back(a, q.nullHandlingEnabled);
    std::vector<const char*> key_names;
    for (const auto& g : q.groupByExpressions) key_names.push_back(g.c_str());
    const bool grouped = !q.groupByExpressions.empty();
    std::vector<ResultsBlock> blocks;
    int64_t row = 0;
    for (int b = 0; b < num_blocks; ++b) {
      if (!grouped && block_rows[b] != 1) throw QueryException("an aggregation-only block has one row");
      ResultsBlock block = blockFromArrays(grouped, functions, (int32_t)key_names.size(), key_names.data(), key_types, row, row + block_rows[b], key_longs, key_doubles,
                                           key_strings, key_is_null, counts, sums, mins, maxs, is_null, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, m2s);
      if (grouped) trimSegmentGroupByBlock(&block, q);
      blocks.push_back(std::move(block));
      row += block_rows[b];
    }
    if (blocks.empty()) throw QueryException("no blocks");
    std::ostringstream o;
    if (!grouped) {
      ResultsBlock merged = blocks[0];
      for (size_t i = 1; i < blocks.size(); ++i) mergeResultsBlocks(&merged, blocks[i]);
      o << "{\"combined\": " << blockJson(merged) << "}";
    } else {
      const ResultsBlock combined = combineGroupByBlocks(blocks, q);
      const std::vector<ReducedRow> reduced = reduceGroupBy(combined, q);
      o << "{\"combined\": " << blockJson(combined) << ", \"reduced\": " << reducedJson(reduced) << ", \"resultTable\": " << resultTableJson(toResultTable(reduced, combined, q)) << "}";
    }
    out = o.str();
  });
  return *status == 0 ? strdup(out.c_str()) : nullptr;
}
// HyperLogLog.cardinality() of 2^log2m registers (pinot_amd/csrc/pg_hll.h); -1: not a register count the sketch has, or a rank it cannot hold
int64_t ph_hll_cardinality(const uint8_t* registers, int32_t num_registers) {
  if (!registers || num_registers < (1 << PG_HLL_MIN_LOG2M) || num_registers > (1 << PG_HLL_MAX_LOG2M) || (num_registers & (num_registers - 1)) != 0) return -1;
  int64_t out = -1;
  (void)guarded([&] { out = HllRegisters::fromDeviceRegisters(registers, num_registers).cardinality(); });
  return out;
}
// The registers after offering `num` longs to an empty sketch of 2^log2m registers, with the hash / index / rank of pinot_amd/csrc/pg_hll.h -- the
// header the kernels include -- so that CPU tests hold that arithmetic to the numpy model.  out_registers: 2^log2m bytes.  Returns 0, or 1 for a bad log2m.
int32_t ph_hll_offer_longs(const int64_t* longs, int64_t num, int32_t log2m, uint8_t* out_registers) {
  if (log2m < PG_HLL_MIN_LOG2M || log2m > PG_HLL_MAX_LOG2M || !out_registers || (num > 0 && !longs)) return 1;
  memset(out_registers, 0, (size_t)1 << log2m);
  for (int64_t i = 0; i < num; ++i) {
    const uint32_t x = pg::hll_hash_long((uint64_t)longs[i]);
    uint8_t& reg = out_registers[pg::hll_index(x, log2m)];
    reg = std::max(reg, (uint8_t)pg::hll_rank(x, log2m));
  }
  return 0;
}
// hll_float_bits_of_widened of the same header: the 32 stored bits of a FLOAT dictionary entry from the bits of the double it was widened to
uint32_t ph_hll_float_bits_of_widened(uint64_t double_bits) { return pg::hll_float_bits_of_widened(double_bits); }

// The host side of pg_result_value_counts without a device (CPU tests, the stand-alone sanitizer program): the runs of a raw column as the
// intermediate results that segments merge.  stored_type: 0 INT, 1 LONG, 2 FLOAT, 3 DOUBLE; the out arrays hold `num` entries; returns how many were written.
int32_t ph_value_counts_from_device(int32_t stored_type, const int64_t* value_bits, const uint32_t* counts, int32_t num, double* out_values, int64_t* out_counts) {
  const ValueCounts list = ValueCounts::fromDeviceValues((DataType)stored_type, value_bits, counts, num);
  for (size_t i = 0; i < list.values.size(); ++i) { out_values[i] = list.values[i]; out_counts[i] = list.counts[i]; }
  return (int32_t)list.values.size();
}
int32_t ph_value_set_from_device(int32_t stored_type, const int64_t* value_bits, int32_t num, int64_t* out_values) {
  const ValueSet set = ValueSet::fromDeviceValues((DataType)stored_type, value_bits, num);
  for (size_t i = 0; i < set.values.size(); ++i) out_values[i] = set.values[i];
  return (int32_t)set.values.size();
}

// GroupByUtils.getTableCapacity / getIndexedTableTrimThreshold (core/util/GroupByUtils.java:48-73)
int32_t ph_group_by_table_capacity(int32_t limit, int32_t min_num_groups) { return GroupByUtils::getTableCapacity(limit, min_num_groups); }
int32_t ph_group_by_trim_threshold(int32_t trim_size, int32_t trim_threshold) { return GroupByUtils::getIndexedTableTrimThreshold(trim_size, trim_threshold); }

// The host decoder of pg_chunk_codec.h (what pg_segment_open runs under PINOT_GPU_CHUNK_DECODE=host and for chunks above the device cap; the device
// kernel walks the same parsers).  codec: ChunkCompressionType value, 1 SNAPPY | 3 LZ4; `dst` has exactly `expect` bytes.  Returns 1 (pgcodec::kEnd)
// when the chunk decoded to exactly `expect` bytes, otherwise the parser's error code (2..10).
int32_t ph_chunk_decode(int32_t codec, const uint8_t* src, uint32_t size, uint8_t* dst, uint32_t expect) {
  return pgcodec::decode_chunk_host(codec, src, size, dst, expect);
}
// A whole LZ4 / SNAPPY fixed-byte chunk file (versions 1 to 4) of `num_docs` docs -> its num_docs * sizeOfEntry value bytes, big-endian as stored.
// Returns 0; 1: the header or the offset table fails the checks made before any chunk is decoded (ph_last_error says which); 2: a codec that is
// not decoded here; 3: a malformed chunk.
int32_t ph_raw_decode_file(const uint8_t* file, uint64_t size, int64_t num_docs, uint8_t* out_values) {
  pgcodec::ChunkFile cf;
  int r = pgcodec::parse_chunk_header(file, size, &cf);
  if (r == pgcodec::kFileOk && cf.codec != pgcodec::kLz4 && cf.codec != pgcodec::kSnappy) {
    g_hostError = std::string("compressionType ") + pgcodec::codec_name(cf.codec) + " is not decoded";
    return 2;
  }
  if (r == pgcodec::kFileOk) r = pgcodec::validate_chunk_table(cf, file, size, num_docs);
  if (r != pgcodec::kFileOk) {
    g_hostError = r == pgcodec::kFileBadOffsets ? "chunk offsets decrease or point outside the file" : r == pgcodec::kFileBadChunkCount ? "numChunks does not match numDocs and numDocsPerChunk"
                  : r == pgcodec::kFileTruncated ? "header or offset table truncated" : "bad header";
    return 1;
  }
  int bad = 0;
  r = pgcodec::decode_file_host(cf, file, size, num_docs, out_values, &bad);
  if (r != pgcodec::kEnd) { g_hostError = "chunk " + std::to_string(bad) + " is malformed (error " + std::to_string(r) + ")"; return 3; }
  return 0;
}

}  // extern "C"
