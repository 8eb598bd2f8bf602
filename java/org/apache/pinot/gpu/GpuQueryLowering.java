/**
 * Lowers a QueryContext over one segment into the flat arrays of jni/pg_marshal.h -- or says the query keeps the CPU plan.
 *
 * <p>The filter is lowered into the PHYSICAL operator tree the reference itself would build: FilterPlanNode.constructPhysicalOperator
 * calls FilterOperatorUtils.get{Leaf,And,Or,Not}FilterOperator (core/operator/filter/FilterOperatorUtils.java:68-193), which pick the
 * leaf operator from the column's indexes, drop MatchAll / Empty children and re-order the children of an AND by priority (:196-245).
 * The order travels with the query: AndDocIdSet.iterator() applies scan-based children in list order, and the engine's
 * numEntriesScannedInFilter follows it.  The predicates are evaluated by the reference's own PredicateEvaluators: this class only reads
 * what they decided (always true / false, dictId range, matching dictIds), it never compares values itself -- except for raw
 * (no-dictionary) columns, whose evaluators are private classes: there the inclusive bounds are derived from the RangePredicate /
 * EqPredicate strings with the same java.lang parsers the evaluators use.
 *
 * <p>C++ twin (tested here, where no JDK exists): pinot_amd/csrc/host/plan_maker.cpp, lowerFilter / physAnd / physOr / physNot.
 */
package org.apache.pinot.gpu;

import java.util.ArrayList;
import java.util.Arrays;
import java.util.List;
import java.util.Map;
import javax.annotation.Nullable;
import org.apache.pinot.common.request.context.ExpressionContext;
import org.apache.pinot.common.request.context.FilterContext;
import org.apache.pinot.common.request.context.predicate.BaseInPredicate;
import org.apache.pinot.common.request.context.predicate.EqPredicate;
import org.apache.pinot.common.request.context.predicate.NotEqPredicate;
import org.apache.pinot.common.request.context.predicate.Predicate;
import org.apache.pinot.common.request.context.predicate.RangePredicate;
import org.apache.pinot.core.operator.filter.predicate.PredicateEvaluator;
import org.apache.pinot.core.operator.filter.predicate.PredicateEvaluatorProvider;
import org.apache.pinot.core.operator.filter.predicate.RangePredicateEvaluatorFactory.SortedDictionaryBasedRangePredicateEvaluator;
import org.apache.pinot.core.query.aggregation.function.AggregationFunction;
import org.apache.pinot.core.query.aggregation.function.DistinctCountHLLAggregationFunction;
import org.apache.pinot.core.query.request.context.QueryContext;
import org.apache.pinot.segment.spi.IndexSegment;
import org.apache.pinot.segment.spi.datasource.DataSource;
import org.apache.pinot.segment.spi.index.reader.NullValueVectorReader;
import org.apache.pinot.segment.spi.index.reader.SortedIndexReader;
import org.apache.pinot.spi.data.FieldSpec.DataType;
import org.apache.pinot.spi.utils.Pairs;
import org.roaringbitmap.buffer.ImmutableRoaringBitmap;


final class GpuQueryLowering {
  // pg_predicate_kind / pg_leaf_eval / pg_filter_op / pg_agg_function: the numbers live in PinotGpuNative, next to the header they mirror
  static final int PRED_MATCH_ALL = PinotGpuNative.PG_PRED_MATCH_ALL;
  static final int PRED_MATCH_NONE = PinotGpuNative.PG_PRED_MATCH_NONE;
  static final int PRED_DICT_RANGE = PinotGpuNative.PG_PRED_DICT_RANGE;
  static final int PRED_DICT_SET = PinotGpuNative.PG_PRED_DICT_SET;
  static final int PRED_RAW_RANGE = PinotGpuNative.PG_PRED_RAW_RANGE;
  static final int PRED_RAW_SET = PinotGpuNative.PG_PRED_RAW_SET;
  static final int PRED_DOC_RANGE = PinotGpuNative.PG_PRED_DOC_RANGE;
  static final int PRED_IS_NULL = PinotGpuNative.PG_PRED_IS_NULL;
  static final int PRED_DOC_SET = PinotGpuNative.PG_PRED_DOC_SET;
  static final int EVAL_SCAN = PinotGpuNative.PG_EVAL_SCAN;
  static final int EVAL_INVERTED = PinotGpuNative.PG_EVAL_INVERTED;
  static final int OP_LEAF = PinotGpuNative.PG_FILTER_LEAF;
  static final int OP_AND = PinotGpuNative.PG_FILTER_AND;
  static final int OP_OR = PinotGpuNative.PG_FILTER_OR;
  static final int OP_NOT = PinotGpuNative.PG_FILTER_NOT;
  static final int AGG_COUNT = PinotGpuNative.PG_AGG_COUNT;
  static final int AGG_SUM = PinotGpuNative.PG_AGG_SUM;
  static final int AGG_MIN = PinotGpuNative.PG_AGG_MIN;
  static final int AGG_MAX = PinotGpuNative.PG_AGG_MAX;
  static final int AGG_AVG = PinotGpuNative.PG_AGG_AVG;
  static final int AGG_DISTINCTCOUNT = PinotGpuNative.PG_AGG_DISTINCTCOUNT;
  static final int AGG_PERCENTILE = PinotGpuNative.PG_AGG_PERCENTILE;
  static final int AGG_DISTINCTCOUNTHLL = PinotGpuNative.PG_AGG_DISTINCTCOUNTHLL;
  static final int AGG_VARIANCE = PinotGpuNative.PG_AGG_VARIANCE;
  private static final int NODE_INTS = PinotGpuNative.PGM_FILTER_NODE_INTS;
  private static final int PRED_INTS = PinotGpuNative.PGM_PRED_INTS;
  private static final int PRED_LONGS = PinotGpuNative.PGM_PRED_LONGS;
  private static final int AGG_INTS = PinotGpuNative.PGM_AGG_INTS;

  // PrioritizedFilterOperator.java:32-39
  private static final int SORTED_PRIORITY = 0;
  private static final int BITMAP_PRIORITY = 100;
  private static final int AND_PRIORITY = 300;
  private static final int OR_PRIORITY = 400;
  private static final int SCAN_PRIORITY = 500;
  private static final int UNKNOWN_PRIORITY = 10000;

  /** The arrays PinotGpuNative.queryCheck / execute take. */
  static final class Lowered {
    int[] _filterNodes;
    int[] _predInts;
    long[] _predLongs;
    int[] _setOffsets;
    int[] _setWords;
    int[] _aggregations;
    int[] _groupBy;
    int _numGroupsLimit;
    int _flags;
    boolean _hasDistinctCount;      // a DISTINCTCOUNT among the aggregations: executed alone through executeWithDistinctSets, never in a batch
    boolean _hasPercentile;         // a PERCENTILE among the aggregations: executed alone through executeWithPercentileCounts, never in a batch
    boolean _hasMoments;            // a VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP among the aggregations: executed alone through executeWithMoments, never in a batch
    boolean _hasHll;                // a DISTINCTCOUNTHLL among the aggregations: executed alone through executeWithHllRegisters, never in a batch
    boolean _rawValueLists;         // those DISTINCTCOUNT / PERCENTILE columns are RAW (no dictionary): executed through executeWithValueLists instead
  }

  /** Thrown inside the lowering when a construct has no device form; the plan maker keeps the CPU plan. */
  static final class NotOffloadable extends RuntimeException {
    NotOffloadable(String why) {
      super(why, null, false, false);
    }
  }

  private enum Kind { MATCH_ALL, EMPTY, LEAF, AND, OR, NOT }

  private static final class Node {
    Kind _kind = Kind.LEAF;
    int _predicate = -1;
    int _priority = UNKNOWN_PRIORITY;
    List<Node> _children = new ArrayList<>();
  }

  private final GpuSegment _segment;
  private final IndexSegment _indexSegment;
  private final QueryContext _queryContext;
  private final List<int[]> _predInts = new ArrayList<>();
  private final List<long[]> _predLongs = new ArrayList<>();
  private final List<int[]> _predSets = new ArrayList<>();
  private long _docSetId;                    // the doc set of the segment's queryable docIds (upsert / dedup tables), or 0

  // gpu.exact.filter.stats of the plan maker's configuration (GpuPlanMaker.init); a query turns it off for itself with the option gpuExactFilterStats=false
  private static volatile boolean _exactFilterStats = true;

  static void setExactFilterStats(boolean exact) {
    _exactFilterStats = exact;
  }

  /** PG_QUERY_STATS_UPPER_BOUND_OK for this query: the server's setting, or the query's own option. */
  static boolean statsUpperBoundOk(QueryContext queryContext) {
    if (!_exactFilterStats) {
      return true;
    }
    Map<String, String> options = queryContext.getQueryOptions();
    String option = options == null ? null : options.get(GpuPlanMaker.EXACT_FILTER_STATS_QUERY_OPTION);
    return option != null && "false".equalsIgnoreCase(option.trim());
  }

  private GpuQueryLowering(GpuSegment segment, IndexSegment indexSegment, QueryContext queryContext) {
    _segment = segment;
    _indexSegment = indexSegment;          // handed in per query: the device copy keeps no reference to the IndexSegment (GpuSegmentCache)
    _queryContext = queryContext;
  }

  /** The lowered query, or null when it keeps the CPU plan (the reason is logged by the caller at debug level). */
  @Nullable
  static Lowered lower(GpuSegment segment, IndexSegment indexSegment, QueryContext queryContext, AggregationFunction[] functions,
      @Nullable FilterContext filter) {
    try {
      return new GpuQueryLowering(segment, indexSegment, queryContext).run(functions, filter);
    } catch (NotOffloadable e) {
      return null;
    }
  }

  /**
   * The same for a segment of an upsert / dedup table: {@code docSetId} names the doc set of its queryable docIds, and the filter becomes
   * FilterPlanNode.run()'s (:88-106) AND(user filter, valid docs) -- the leaf alone without a user filter.
   */
  @Nullable
  static Lowered lowerWithDocSet(GpuSegment segment, IndexSegment indexSegment, QueryContext queryContext, AggregationFunction[] functions,
      @Nullable FilterContext filter, long docSetId) {
    try {
      GpuQueryLowering lowering = new GpuQueryLowering(segment, indexSegment, queryContext);
      lowering._docSetId = docSetId;
      return lowering.run(functions, filter);
    } catch (NotOffloadable e) {
      return null;
    }
  }

  /**
   * What a FILTER (WHERE ...) clause folds to on this segment: +1 matches every doc (MatchAllFilterOperator), -1 matches none
   * (EmptyFilterOperator), 0 neither.  AggregationFunctionUtils.buildFilteredAggregationInfos (:351-358, :376-378) treats the functions of
   * a match-all clause as non-filtered; the plan maker does the same with this answer.  Null when the clause has no device form.
   */
  @Nullable
  static Integer foldsTo(GpuSegment segment, IndexSegment indexSegment, QueryContext queryContext, FilterContext filter) {
    try {
      Node root = new GpuQueryLowering(segment, indexSegment, queryContext).lowerFilter(filter);
      return root._kind == Kind.MATCH_ALL ? 1 : (root._kind == Kind.EMPTY ? -1 : 0);
    } catch (NotOffloadable e) {
      return null;
    }
  }

  private Lowered run(AggregationFunction[] functions, @Nullable FilterContext filter) {
    Lowered out = new Lowered();
    // ---- aggregations: COUNT / SUM / MIN / MAX / AVG over one identifier (AggregationFunctionType) ----
    // (no functions at all: the group-by lane FilteredGroupByOperator runs over the main filter only to create its groups,
    //  AggregationFunctionUtils.java:388-400 -- the device needs something to aggregate, so it counts; the operator ignores the value)
    out._aggregations = functions.length == 0 ? new int[]{AGG_COUNT, -1} : new int[AGG_INTS * functions.length];
    for (int i = 0; i < functions.length; i++) {
      AggregationFunction function = functions[i];
      int code;
      switch (function.getType()) {
        case COUNT:
          code = AGG_COUNT;
          break;
        case SUM:
          code = AGG_SUM;
          break;
        case MIN:
          code = AGG_MIN;
          break;
        case MAX:
          code = AGG_MAX;
          break;
        case AVG:
          code = AGG_AVG;
          break;
        case DISTINCTCOUNT:
          code = AGG_DISTINCTCOUNT;
          break;
        case DISTINCTCOUNTHLL: {
          // the HyperLogLog registers are built on the device, whichever way the column is stored; log2m travels in the function word
          int log2m = ((DistinctCountHLLAggregationFunction) function).getLog2m();
          if (log2m < PinotGpuNative.PG_HLL_MIN_LOG2M || log2m > PinotGpuNative.PG_HLL_MAX_LOG2M) {
            throw new NotOffloadable("DISTINCTCOUNTHLL with log2m " + log2m);
          }
          code = PinotGpuNative.hllFunctionWord(log2m);
          out._hasHll = true;
          break;
        }
        case VARPOP:
        case VARSAMP:
        case STDDEVPOP:
        case STDDEVSAMP:
          // VarianceAggregationFunction: one intermediate for all four, VarianceTuple(count, sum, m2); the final value stays with the function object
          code = AGG_VARIANCE;
          out._hasMoments = true;
          break;
        case PERCENTILE:
          // the exact PercentileAggregationFunction (PERCENTILE50(col) / PERCENTILE(col, 50)); the percentile itself stays with the function object:
          // the device returns the whole value list whatever it is
          code = AGG_PERCENTILE;
          break;
        default:
          throw new NotOffloadable("aggregation function " + function.getType());
      }
      int column = -1;
      List<ExpressionContext> inputs = function.getInputExpressions();
      if (code == AGG_COUNT) {
        // COUNT(col) is COUNT(*) unless null handling is on (CountAggregationFunction.java:44-50)
        if (_queryContext.isNullHandlingEnabled() && !inputs.isEmpty() && inputs.get(0).getType() == ExpressionContext.Type.IDENTIFIER
            && !"*".equals(inputs.get(0).getIdentifier())) {
          column = _segment.columnIndex(inputs.get(0).getIdentifier());
        }
      } else {
        if (inputs.size() != 1 || inputs.get(0).getType() != ExpressionContext.Type.IDENTIFIER) {
          throw new NotOffloadable("aggregation over an expression");
        }
        column = _segment.columnIndex(inputs.get(0).getIdentifier());
        if (!_segment.isNumeric(column)) {
          throw new NotOffloadable("aggregation of a non-numeric column");   // the reference throws BadQueryRequestException itself
        }
        if (code == AGG_DISTINCTCOUNT || code == AGG_PERCENTILE) {
          // a dictionary column: dictId bitsets / dictId count histograms on the device; a raw INT / LONG / FLOAT / DOUBLE column: the matching docs'
          // values collected, sorted and run-length encoded (PinotGpuNative.executeWithValueLists).  One query takes one of the two forms: the engine
          // declines a mix, and so does this lowering
          boolean raw = !_segment.hasDictionary(column);
          if ((out._hasDistinctCount || out._hasPercentile) && raw != out._rawValueLists) {
            throw new NotOffloadable("DISTINCTCOUNT / PERCENTILE on raw and dictionary columns in one query");
          }
          out._rawValueLists = raw;
          if (code == AGG_DISTINCTCOUNT) {
            out._hasDistinctCount = true;
          } else {
            out._hasPercentile = true;
          }
        }
      }
      out._aggregations[AGG_INTS * i] = code;
      out._aggregations[AGG_INTS * i + 1] = column;
    }
    if (out._hasHll && (out._hasDistinctCount || out._hasPercentile)) {
      // one native call returns one kind of intermediate result (and the engine declines most of these mixes itself)
      throw new NotOffloadable("DISTINCTCOUNTHLL beside DISTINCTCOUNT / PERCENTILE in one query");
    }
    if (out._hasMoments && (out._hasDistinctCount || out._hasPercentile || out._hasHll)) {
      throw new NotOffloadable("a variance function beside DISTINCTCOUNT / PERCENTILE / DISTINCTCOUNTHLL in one query");
    }
    // ---- group-by keys: dictionary-encoded identifiers ----
    List<ExpressionContext> groupBy = _queryContext.getGroupByExpressions();
    out._groupBy = new int[groupBy == null ? 0 : groupBy.size()];
    for (int i = 0; i < out._groupBy.length; i++) {
      ExpressionContext expression = groupBy.get(i);
      if (expression.getType() != ExpressionContext.Type.IDENTIFIER) {
        throw new NotOffloadable("group-by over an expression");
      }
      int column = _segment.columnIndex(expression.getIdentifier());
      if (!_segment.hasDictionary(column)) {
        // DefaultGroupByExecutor.java:106-121: the no-dictionary key generators (keys by value).  The device groups a raw INT / LONG
        // column through its key image (value - min as the dictId, include/pinot_gpu.h pg_group_key_info); whether the column's value
        // range allows one is pg_query_check's decision (GpuPlanMaker keeps the CPU plan on PG_ERR_UNSUPPORTED).
        // (round 5: FLOAT / DOUBLE columns and INT / LONG columns over more than an int too -- through a dictionary the device builds from
        //  the column's own values, PinotGpuNative.groupKeyValues; STRING / BYTES raw keys keep the CPU plan)
        DataType storedType = _indexSegment.getDataSource(expression.getIdentifier()).getDataSourceMetadata().getDataType().getStoredType();
        if (storedType != DataType.INT && storedType != DataType.LONG && storedType != DataType.FLOAT && storedType != DataType.DOUBLE) {
          throw new NotOffloadable("group-by on a raw " + storedType + " column (NoDictionary key generators)");
        }
      }
      out._groupBy[i] = column;
    }
    // ---- filter ----
    List<int[]> nodes = new ArrayList<>();
    if (_docSetId != 0) {
      // FilterPlanNode.java:92-103: getAndFilterOperator(Arrays.asList(filterOperator, validDocFilter)) -- in that child order, re-ordered
      // by priority like every AND (the bitmap leaf has priority 100); without a filter the BitmapBasedFilterOperator is the whole filter
      Node valid = leaf(PRED_DOC_SET, -1, EVAL_SCAN, false, _docSetId, 0, null, BITMAP_PRIORITY);
      Node root = filter != null ? and(new ArrayList<>(Arrays.asList(lowerFilter(filter), valid))) : valid;
      if (root._kind == Kind.EMPTY) {              // the user filter matches nothing on this segment: EmptyFilterOperator
        root = leaf(PRED_MATCH_NONE, -1, EVAL_SCAN, false, 0, 0, null, UNKNOWN_PRIORITY);
      }
      flatten(root, nodes);
    } else if (filter != null) {
      Node root = lowerFilter(filter);
      if (root._kind != Kind.MATCH_ALL) {          // a filter that matches everything is no filter (MatchAllFilterOperator)
        flatten(root, nodes);
      }
    }
    out._filterNodes = new int[NODE_INTS * nodes.size()];
    for (int i = 0; i < nodes.size(); i++) {
      System.arraycopy(nodes.get(i), 0, out._filterNodes, NODE_INTS * i, NODE_INTS);
    }
    int numPredicates = _predInts.size();
    out._predInts = new int[PRED_INTS * numPredicates];
    out._predLongs = new long[PRED_LONGS * numPredicates];
    out._setOffsets = new int[numPredicates + 1];
    int totalWords = 0;
    for (int[] set : _predSets) {
      totalWords += set.length;
    }
    out._setWords = new int[totalWords];
    int at = 0;
    for (int i = 0; i < numPredicates; i++) {
      System.arraycopy(_predInts.get(i), 0, out._predInts, PRED_INTS * i, PRED_INTS);
      System.arraycopy(_predLongs.get(i), 0, out._predLongs, PRED_LONGS * i, PRED_LONGS);
      int[] set = _predSets.get(i);
      System.arraycopy(set, 0, out._setWords, at, set.length);
      at += set.length;
      out._setOffsets[i + 1] = at;
    }
    out._numGroupsLimit = _queryContext.getNumGroupsLimit();
    out._flags = (_queryContext.isNullHandlingEnabled() ? PinotGpuNative.PG_QUERY_NULL_HANDLING : 0)
        | (statsUpperBoundOk(_queryContext) ? PinotGpuNative.PG_QUERY_STATS_UPPER_BOUND_OK : 0);
    return out;
  }

  // ---- the physical tree: FilterOperatorUtils.getAndFilterOperator / getOrFilterOperator / getNotFilterOperator ----

  private static Node constant(boolean all) {
    Node n = new Node();
    n._kind = all ? Kind.MATCH_ALL : Kind.EMPTY;
    return n;
  }

  private static Node and(List<Node> children) {
    List<Node> kept = new ArrayList<>();
    for (Node child : children) {
      if (child._kind == Kind.EMPTY) {
        return constant(false);
      }
      if (child._kind != Kind.MATCH_ALL) {
        kept.add(child);
      }
    }
    if (kept.isEmpty()) {
      return constant(true);
    }
    if (kept.size() == 1) {
      return kept.get(0);
    }
    kept.sort((a, b) -> Integer.compare(a._priority, b._priority));        // List.sort is stable, like the reference's
    Node n = new Node();
    n._kind = Kind.AND;
    n._priority = AND_PRIORITY;
    n._children = kept;
    return n;
  }

  private static Node or(List<Node> children) {
    List<Node> kept = new ArrayList<>();
    for (Node child : children) {
      if (child._kind == Kind.MATCH_ALL) {
        return constant(true);
      }
      if (child._kind != Kind.EMPTY) {
        kept.add(child);
      }
    }
    if (kept.isEmpty()) {
      return constant(false);
    }
    if (kept.size() == 1) {
      return kept.get(0);
    }
    Node n = new Node();
    n._kind = Kind.OR;
    n._priority = OR_PRIORITY;
    n._children = kept;
    return n;
  }

  private static Node not(Node child) {
    if (child._kind == Kind.MATCH_ALL) {
      return constant(false);
    }
    if (child._kind == Kind.EMPTY) {
      return constant(true);
    }
    Node n = new Node();
    n._kind = Kind.NOT;
    n._priority = child._priority;             // getPriority(NotFilterOperator) = priority of its child (:228-230)
    n._children.add(child);
    return n;
  }

  private Node leaf(int kind, int column, int eval, boolean exclusive, long lo, long hi, int[] setWords, int priority) {
    _predInts.add(new int[]{kind, column, eval, exclusive ? 1 : 0});
    _predLongs.add(new long[]{lo, hi});
    _predSets.add(setWords == null ? new int[0] : setWords);
    Node n = new Node();
    n._kind = Kind.LEAF;
    n._predicate = _predInts.size() - 1;
    n._priority = priority;
    return n;
  }

  private Node lowerFilter(FilterContext filter) {
    switch (filter.getType()) {
      case AND: {
        List<Node> children = new ArrayList<>();
        for (FilterContext child : filter.getChildren()) {
          children.add(lowerFilter(child));
        }
        return and(children);
      }
      case OR: {
        List<Node> children = new ArrayList<>();
        for (FilterContext child : filter.getChildren()) {
          children.add(lowerFilter(child));
        }
        return or(children);
      }
      case NOT:
        return not(lowerFilter(filter.getChildren().get(0)));
      case CONSTANT:
        return constant(filter.isConstantTrue());
      case PREDICATE:
        return lowerPredicate(filter.getPredicate());
      default:
        throw new NotOffloadable("filter type " + filter.getType());
    }
  }

  private Node lowerPredicate(Predicate predicate) {
    ExpressionContext lhs = predicate.getLhs();
    if (lhs.getType() != ExpressionContext.Type.IDENTIFIER) {
      throw new NotOffloadable("predicate over an expression");
    }
    String columnName = lhs.getIdentifier();
    int column = _segment.columnIndex(columnName);
    DataSource dataSource = _indexSegment.getDataSource(columnName);
    boolean hasNulls = hasNulls(dataSource);
    Predicate.Type type = predicate.getType();
    if (type == Predicate.Type.IS_NULL || type == Predicate.Type.IS_NOT_NULL) {
      // FilterPlanNode.java:294-310: the null bitmap as a BitmapBasedFilterOperator; Empty / MatchAll without a null vector
      if (!hasNulls) {
        return constant(type == Predicate.Type.IS_NOT_NULL);
      }
      return leaf(PRED_IS_NULL, column, EVAL_SCAN, type == Predicate.Type.IS_NOT_NULL, 0, 0, null, BITMAP_PRIORITY);
    }
    if (type != Predicate.Type.EQ && type != Predicate.Type.NOT_EQ && type != Predicate.Type.IN && type != Predicate.Type.NOT_IN
        && type != Predicate.Type.RANGE) {
      throw new NotOffloadable("predicate type " + type);
    }
    if (!_segment.hasDictionary(column)) {
      return lowerRawPredicate(predicate, column, dataSource);
    }
    PredicateEvaluator evaluator = PredicateEvaluatorProvider.getPredicateEvaluator(predicate, dataSource, _queryContext);
    if (evaluator.isAlwaysFalse()) {
      return constant(false);                                                              // EmptyFilterOperator (FilterOperatorUtils.java:72-73)
    }
    if (evaluator.isAlwaysTrue()) {
      if (_queryContext.isNullHandlingEnabled() && hasNulls) {
        return leaf(PRED_IS_NULL, column, EVAL_SCAN, true, 0, 0, null, BITMAP_PRIORITY);   // :75-86
      }
      return constant(true);
    }
    int cardinality = dataSource.getDataSourceMetadata().getCardinality();
    boolean exclusive = evaluator.isExclusive();
    boolean isRange = evaluator instanceof SortedDictionaryBasedRangePredicateEvaluator;
    int start = 0;
    int end = 0;
    int[] dictIds = null;
    if (isRange) {
      start = ((SortedDictionaryBasedRangePredicateEvaluator) evaluator).getStartDictId();
      end = ((SortedDictionaryBasedRangePredicateEvaluator) evaluator).getEndDictId();
    } else if (type == Predicate.Type.RANGE) {
      throw new NotOffloadable("range predicate on an unsorted dictionary");
    } else {
      dictIds = exclusive ? evaluator.getNonMatchingDictIds() : evaluator.getMatchingDictIds();
      dictIds = dictIds.clone();
      Arrays.sort(dictIds);
      if (dictIds.length == 1) {
        isRange = true;                                                                    // EQ / NOT_EQ: the dictId range [d, d + 1)
        start = dictIds[0];
        end = start + 1;
      }
    }
    boolean sorted = dataSource.getDataSourceMetadata().isSorted() && dataSource.getInvertedIndex() instanceof SortedIndexReader;
    if (sorted) {
      // SortedIndexBasedFilterOperator (priority 0, :96-104, :123-126): docId ranges of the matching dictIds, adjacent ones merged,
      // complemented over [0, numDocs) for exclusive predicates (SortedIndexBasedFilterOperator.java:60-125)
      SortedIndexReader<?> sortedIndex = (SortedIndexReader<?>) dataSource.getInvertedIndex();
      List<int[]> ranges = new ArrayList<>();
      if (isRange) {
        ranges.add(new int[]{sortedIndex.getDocIds(start).getLeft(), sortedIndex.getDocIds(end - 1).getRight()});
      } else {
        for (int dictId : dictIds) {
          Pairs.IntPair pair = sortedIndex.getDocIds(dictId);
          if (!ranges.isEmpty() && pair.getLeft() == ranges.get(ranges.size() - 1)[1] + 1) {
            ranges.get(ranges.size() - 1)[1] = pair.getRight();
          } else {
            ranges.add(new int[]{pair.getLeft(), pair.getRight()});
          }
        }
      }
      if (exclusive) {
        List<int[]> rest = new ArrayList<>();
        int next = 0;
        int numDocs = _segment.numDocs();
        for (int[] range : ranges) {
          if (range[0] > next) {
            rest.add(new int[]{next, range[0] - 1});
          }
          next = range[1] + 1;
        }
        if (next < numDocs) {
          rest.add(new int[]{next, numDocs - 1});
        }
        ranges = rest;
        if (ranges.isEmpty()) {
          return constant(false);
        }
      }
      List<Node> leaves = new ArrayList<>();
      for (int[] range : ranges) {
        leaves.add(leaf(PRED_DOC_RANGE, column, EVAL_SCAN, false, range[0], range[1], null, SORTED_PRIORITY));
      }
      if (leaves.size() == 1) {
        return leaves.get(0);
      }
      Node n = new Node();                       // ONE sorted operator in the reference: an OR the iterators merge back (OrDocIdSet.java:94-112)
      n._kind = Kind.OR;
      n._priority = SORTED_PRIORITY;
      n._children = leaves;
      return n;
    }
    // :106-133: RANGE predicates scan (no range index on this path); every other type prefers the inverted index.
    // InvertedIndexFilterOperator is none of the classes reorderAndFilterChildOperators knows: it sorts last.
    boolean inverted = type != Predicate.Type.RANGE && dataSource.getInvertedIndex() != null;
    int eval = inverted ? EVAL_INVERTED : EVAL_SCAN;
    int priority = inverted ? UNKNOWN_PRIORITY : SCAN_PRIORITY;
    if (isRange) {
      return leaf(PRED_DICT_RANGE, column, eval, exclusive, start, end, null, priority);
    }
    int[] words = new int[(cardinality + 31) >>> 5];
    for (int dictId : dictIds) {
      words[dictId >>> 5] |= 1 << (dictId & 31);
    }
    return leaf(PRED_DICT_SET, column, eval, exclusive, 0, 0, words, priority);
  }

  /** Raw (no-dictionary) numeric column: RANGE / EQ / NOT_EQ as inclusive bounds, the way the *RawValueBasedRangePredicateEvaluators hold them. */
  private Node lowerRawPredicate(Predicate predicate, int column, DataSource dataSource) {
    DataType storedType = dataSource.getDataSourceMetadata().getDataType().getStoredType();
    String lower;
    String upper;
    boolean lowerInclusive = true;
    boolean upperInclusive = true;
    boolean exclusive = false;
    switch (predicate.getType()) {
      case RANGE: {
        RangePredicate range = (RangePredicate) predicate;
        lower = range.getLowerBound();
        upper = range.getUpperBound();
        lowerInclusive = range.isLowerInclusive();
        upperInclusive = range.isUpperInclusive();
        break;
      }
      case EQ:
        lower = ((EqPredicate) predicate).getValue();
        upper = lower;
        break;
      case NOT_EQ:
        lower = ((NotEqPredicate) predicate).getValue();
        upper = lower;
        exclusive = true;
        break;
      case IN:
      case NOT_IN:
        return lowerRawSetPredicate((BaseInPredicate) predicate, column, storedType);
      default:
        throw new NotOffloadable("predicate type " + predicate.getType() + " on a raw column");
    }
    boolean lowerUnbounded = RangePredicate.UNBOUNDED.equals(lower);
    boolean upperUnbounded = RangePredicate.UNBOUNDED.equals(upper);
    long lo;
    long hi;
    switch (storedType) {
      case INT: {
        // IntRawValueBasedRangePredicateEvaluator (RangePredicateEvaluatorFactory.java:326-380): exclusive bounds move by one
        int l = lowerUnbounded ? Integer.MIN_VALUE : Integer.parseInt(lower);
        int u = upperUnbounded ? Integer.MAX_VALUE : Integer.parseInt(upper);
        if (!lowerUnbounded && !lowerInclusive) {
          if (l == Integer.MAX_VALUE) {
            // Preconditions.checkArgument in the reference's evaluator: the CPU plan raises its "Invalid range"
            throw new NotOffloadable("Invalid range");
          }
          l++;
        }
        if (!upperUnbounded && !upperInclusive) {
          if (u == Integer.MIN_VALUE) {
            throw new NotOffloadable("Invalid range");
          }
          u--;
        }
        lo = l;
        hi = u;
        break;
      }
      case LONG: {
        long l = lowerUnbounded ? Long.MIN_VALUE : Long.parseLong(lower);
        long u = upperUnbounded ? Long.MAX_VALUE : Long.parseLong(upper);
        if (!lowerUnbounded && !lowerInclusive) {
          if (l == Long.MAX_VALUE) {
            // Preconditions.checkArgument in the reference's evaluator: the CPU plan raises its "Invalid range"
            throw new NotOffloadable("Invalid range");
          }
          l++;
        }
        if (!upperUnbounded && !upperInclusive) {
          if (u == Long.MIN_VALUE) {
            throw new NotOffloadable("Invalid range");
          }
          u--;
        }
        lo = l;
        hi = u;
        break;
      }
      case FLOAT: {
        // bounds widen to double exactly; exclusive bounds step with Math.nextUp / nextDown in float precision (:438-492)
        float l = lowerUnbounded ? Float.NEGATIVE_INFINITY : Float.parseFloat(lower);
        float u = upperUnbounded ? Float.POSITIVE_INFINITY : Float.parseFloat(upper);
        if (!lowerUnbounded && !lowerInclusive) {
          float up = Math.nextUp(l);
          if (!(up > l)) {
            // +inf or NaN does not move: Preconditions.checkArgument in the reference's evaluator, left to the CPU plan
            throw new NotOffloadable("Invalid range");
          }
          l = up;
        }
        if (!upperUnbounded && !upperInclusive) {
          float down = Math.nextDown(u);
          if (!(down < u)) {
            throw new NotOffloadable("Invalid range");
          }
          u = down;
        }
        lo = Double.doubleToRawLongBits((double) l);
        hi = Double.doubleToRawLongBits((double) u);
        break;
      }
      case DOUBLE: {
        double l = lowerUnbounded ? Double.NEGATIVE_INFINITY : Double.parseDouble(lower);
        double u = upperUnbounded ? Double.POSITIVE_INFINITY : Double.parseDouble(upper);
        if (!lowerUnbounded && !lowerInclusive) {
          double up = Math.nextUp(l);
          if (!(up > l)) {
            // +inf or NaN does not move: Preconditions.checkArgument in the reference's evaluator, left to the CPU plan
            throw new NotOffloadable("Invalid range");
          }
          l = up;
        }
        if (!upperUnbounded && !upperInclusive) {
          double down = Math.nextDown(u);
          if (!(down < u)) {
            throw new NotOffloadable("Invalid range");
          }
          u = down;
        }
        lo = Double.doubleToRawLongBits(l);
        hi = Double.doubleToRawLongBits(u);
        break;
      }
      default:
        throw new NotOffloadable("predicate on a raw " + storedType + " column");
    }
    return leaf(PRED_RAW_RANGE, column, EVAL_SCAN, exclusive, lo, hi, null, SCAN_PRIORITY);
  }

  /**
   * Raw (no-dictionary) INT / LONG / FLOAT / DOUBLE column, IN / NOT_IN: Int / Long / Float / DoubleRawValueBasedInPredicateEvaluator
   * (InPredicateEvaluatorFactory.java:74-107, :215-380; NotInPredicateEvaluatorFactory negates) -- the literals parsed with the column type's
   * parser into a hash set, applySV = set.contains(value).  PG_PRED_RAW_SET: the distinct values, ascending, two set words each (low word
   * first): the value as a long, or the bits of the value as a double (a FLOAT literal is rounded once, by Float.parseFloat, then widened).
   * A scan leaf.  Kept on the CPU plan: a FLOAT / DOUBLE list with a zero or a NaN (how the reference's hash set treats +0.0 / -0.0 and the
   * NaNs is not settled on the device side; for every other value bit equality and == agree), and more than PG_RAW_SET_MAX_VALUES distinct values.
   */
  private Node lowerRawSetPredicate(BaseInPredicate predicate, int column, DataType storedType) {
    boolean exclusive = predicate.getType() == Predicate.Type.NOT_IN;
    List<String> literals = predicate.getValues();
    long[] values = new long[literals.size()];
    int n = 0;
    for (String literal : literals) {
      switch (storedType) {
        case INT:
          values[n++] = Integer.parseInt(literal);
          break;
        case LONG:
          values[n++] = Long.parseLong(literal);
          break;
        case FLOAT:
        case DOUBLE: {
          double v = storedType == DataType.FLOAT ? (double) Float.parseFloat(literal) : Double.parseDouble(literal);
          if (v != v || v == 0.0) {
            throw new NotOffloadable("IN / NOT_IN list with a zero or a NaN on a raw " + storedType + " column");
          }
          values[n++] = Double.doubleToRawLongBits(v);
          break;
        }
        default:
          throw new NotOffloadable("predicate on a raw " + storedType + " column");
      }
    }
    Arrays.sort(values);
    int distinct = 0;
    for (int i = 0; i < n; i++) {
      if (i == 0 || values[i] != values[i - 1]) {
        values[distinct++] = values[i];
      }
    }
    if (distinct > PinotGpuNative.PG_RAW_SET_MAX_VALUES) {
      throw new NotOffloadable("IN / NOT_IN list of " + distinct + " distinct values on a raw column");
    }
    if (distinct == 0) {
      return constant(exclusive);
    }
    int[] words = new int[PinotGpuNative.PG_RAW_SET_WORDS_PER_VALUE * distinct];
    int w = 0;
    for (int i = 0; i < distinct; i++) {
      words[w++] = (int) values[i];
      words[w++] = (int) (values[i] >>> 32);
    }
    return leaf(PRED_RAW_SET, column, EVAL_SCAN, exclusive, 0, 0, words, SCAN_PRIORITY);
  }

  private static boolean hasNulls(DataSource dataSource) {
    NullValueVectorReader reader = dataSource.getNullValueVector();
    if (reader == null) {
      return false;
    }
    ImmutableRoaringBitmap nulls = reader.getNullBitmap();
    return nulls != null && !nulls.isEmpty();
  }

  private static void flatten(Node node, List<int[]> out) {
    switch (node._kind) {
      case LEAF:
        out.add(new int[]{OP_LEAF, node._predicate, 0});
        return;
      case NOT:
        flatten(node._children.get(0), out);
        out.add(new int[]{OP_NOT, -1, 1});
        return;
      case AND:
      case OR:
        for (Node child : node._children) {
          flatten(child, out);
        }
        out.add(new int[]{node._kind == Kind.AND ? OP_AND : OP_OR, -1, node._children.size()});
        return;
      default:
        throw new IllegalStateException("constant nodes are folded before flattening");
    }
  }
}
