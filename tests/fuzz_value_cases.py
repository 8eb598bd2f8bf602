"""DISTINCTCOUNT / PERCENTILE queries derived from the typed fuzz (tests/fuzz_cases.py), and an EXACT MODEL of what each returns -- shared by
tests/test_fuzz_value_cases_cpu.py (oracle vs. model on everything the oracle knows) and tests/test_gpu_fuzz_values.py (device vs. model and
oracle).  Nothing here needs a GPU or the oracle.  Deterministic in (seed, PINOT_FUZZ_SEED_BASE).

The typed fuzz's random stream is NOT touched: F.make_segment / F.make_queries return what they always did, and every choice made here comes
from a generator of its own, np.random.default_rng([seed, SEED_BASE, SALT]).

Per base FuzzQuery, `derive` gives one query per family (DISTINCTCOUNT, PERCENTILE) -- the engine declines the two in one query -- and, from
an ungrouped base query, about half the time a second, grouped, variant per family over one small dictionary key of the segment:
  * filter: the base query's tree, null handling and numGroupsLimit, unchanged (one Pred object behind two leaves stays one object);
  * 1-4 distinct value columns, all dictionary or all raw (the engine declines a mix), without a null vector under null handling;
  * GROUP BY: the base query's keys that plan_distinct / plan_percentile admit -- dictionary columns or raw columns keyed by offset
    (key_scale() == "offset"), not nullable under null handling, at most 4, truncated until the product of the cardinalities is at most
    the effective numGroupsLimit; no surviving key: the query is ungrouped;
  * beside the value functions, about half the time, the base query's ordinary aggregations that the shape admits (`_extra_ok`: the typed
    fuzz's own rules for a grouped aggregation, applied again because the key set changed) -- the base + pass shape; otherwise the value
    functions and, optionally, COUNT(*) -- without GROUP BY that is the pass alone, which counts docs and filter entries itself;
  * about a third get a valid-doc set ANDed at the root (FilterPlanNode.java:92-103, as doc_set_cases.with_valid): a random mask of
    density 0 / 0.02 / 0.5 / 0.98 / 1, the words and roaring formats in turn.
Skipped, because plan_distinct / plan_percentile decline them by shape: a base query with a raw_range leaf on a raw LONG / FLOAT / DOUBLE
column or any raw_range_f64 leaf.

The model: mask = F.filter_mask(seg, companion) AND the valid mask; per value aggregation -- and per group, keyed by the identity tuple
F.expected uses -- np.unique(ids[docs]) (dictionary DISTINCTCOUNT), np.unique(ids[docs], return_counts=True) (dictionary PERCENTILE),
raw_value_cases.runs_of(values[docs]) (raw: order images, NaN canonical, -0.0 before 0.0, Double.compare's order).  DISTINCTCOUNT over
dictionary columns of a query the reference answers without a scan (AggregationPlanNode.java:98-115: the filter matches everything, no
aggregation argument has null values under null handling, every function is COUNT, DISTINCTCOUNT or a dictionary MIN / MAX) is the WHOLE
dictionary with statistics (docs, 0, 0, docs).  Everything the companion query (value functions turned into COUNT(*)) returns is
F.expected's and the oracle's business; numEntriesScannedPostFilter is numDocsScanned x the distinct columns the ORIGINAL query projects.
A doc set is, for the oracle and F.expected, the twin segment of doc_set_cases: an inverted `= 1` leaf on a synthetic column."""
import copy
import itertools

import numpy as np

import distinct_cases as DC
import doc_set_cases as D
import fuzz_cases as F
import percentile_cases as P
import raw_value_cases as RV
from pinot_amd import query as Q

SALT = 0x56414C
VALUE_FUNCTIONS = (Q.DISTINCTCOUNT, Q.PERCENTILE)
FAMILIES = {Q.DISTINCTCOUNT: "DISTINCTCOUNT", Q.PERCENTILE: "PERCENTILE"}
PERCENTILES = (0, 50, 90, 99, 100)
VALID_DENSITIES = (0.0, 0.02, 0.5, 0.98, 1.0)
MAX_KEYS = 4                     # kMaxDistinctKeys
MAX_VALUE_COLUMNS = 4            # kMaxAggCols
SMALL_KEY = 64                   # the second, grouped, variant takes one dictionary key of at most this cardinality


class ValueQuery:
    """One derived query.  `aggs`: the aggregation list with the value functions in it; `tree`: the user's filter (fuzz_cases tuples);
    `valid`: the valid-doc mask or None, `valid_format` "words" / "roaring"; `variant`: "base" or "small-key"."""

    def __init__(self, base_index, family, raw, aggs, tree, group_by, null_handling, limit, valid, valid_format, variant):
        self.base_index, self.family, self.raw, self.aggs, self.tree = base_index, family, raw, aggs, tree
        self.group_by, self.null_handling, self.limit = group_by, null_handling, limit
        self.valid, self.valid_format, self.variant = valid, valid_format, variant
        self.value_positions = [a for a, (f, _) in enumerate(aggs) if f in VALUE_FUNCTIONS]
        self.value_columns = list(dict.fromkeys(aggs[a][1] for a in self.value_positions))
        self.companion_aggs = [((Q.COUNT, -1) if f in VALUE_FUNCTIONS else (f, c)) for f, c in aggs]
        # the user's part of the companion query: what F.filter_mask evaluates
        self.companion = F.FuzzQuery(self.companion_aggs, tree, group_by, null_handling, limit)
        # plan_distinct / plan_percentile: nothing but the value functions and plain counts, no GROUP BY -- one launch that counts docs and entries itself
        self.counts_only = all(f in VALUE_FUNCTIONS or (f == Q.COUNT and (c < 0 or not null_handling)) for f, c in aggs)

    def _with_leaf(self, aggs, leaf):
        tree = ("leaf", leaf) if self.tree is None else ("and", [self.tree, ("leaf", leaf)])
        return F.FuzzQuery(aggs, tree, self.group_by, self.null_handling, self.limit)

    def device(self, doc_set_id=None, companion=False):
        """The FuzzQuery the engine is handed (companion: with the value functions turned into COUNT(*)); doc_set_id: the id of `valid`."""
        aggs = self.companion_aggs if companion else self.aggs
        if self.valid is None:
            return F.FuzzQuery(aggs, self.tree, self.group_by, self.null_handling, self.limit)
        return self._with_leaf(aggs, D.device_leaf(doc_set_id, 0))

    def twin(self, seg):
        """(segment, companion FuzzQuery) the oracle and F.expected answer: the twin of doc_set_cases when there is a doc set."""
        if self.valid is None:
            return seg, self.companion
        return D.twin_fuzz_segment(seg, [self.valid]), self._with_leaf(self.companion_aggs, D.twin_leaf(len(seg.cols)))

    def leaves(self):
        return self.companion.leaves()

    def describe(self, seg):
        return "base query %d %s (%s %s, n=%d, aggs=%r, group_by=%r, null_handling=%r, limit=%d, leaves=%r, doc set %s)" % (
            self.base_index, self.variant, FAMILIES[self.family], "raw" if self.raw else "dictionary", seg.n,
            [(f, seg.cols[c].kind if c >= 0 else "*") for f, c in self.aggs], [seg.cols[k].kind for k in self.group_by], self.null_handling, self.limit,
            [x.kind for x in self.leaves()], "none" if self.valid is None else "%s %d docs" % (self.valid_format, int(self.valid.sum())))


# ------------------------------------------------------------------------------------------------------------------------------------
# derivation
# ------------------------------------------------------------------------------------------------------------------------------------
def eligible(seg, fq):
    """plan_distinct / plan_percentile evaluate the lane-private filter: no range leaf on a raw LONG / FLOAT / DOUBLE column."""
    return not any(x.kind == "raw_range_f64" or (x.kind == "raw_range" and seg.cols[x.column].is_wide_raw) for x in fq.leaves())


def repaired_keys(seg, fq):
    """The base query's keys that the value passes admit (the module's docstring)."""
    def ok(c):
        if fq.null_handling and c.nulls is not None:
            return False
        return c.is_dict or c.key_scale()[0] == "offset"
    keys = [g for g in fq.group_by if ok(seg.cols[g])][:MAX_KEYS]
    limit = fq.limit if fq.limit > 0 else F.DEFAULT_GROUPS_LIMIT
    while keys and int(np.prod([seg.cols[g].key_scale()[2] for g in keys], dtype=object)) > limit:
        keys.pop()
    return keys


def _extra_ok(seg, f, c, grouped, null_handling):
    """An ordinary aggregation of the base query beside the value functions: fuzz_cases._make_query's rules for the key set the derived query has."""
    if c < 0 or not grouped:
        return True
    col = seg.cols[c]
    if f in (Q.SUM, Q.AVG) and col.kind in (F.DICT_LONG, F.RAW_LONG) and not col.sum_safe:
        return False                  # "group-by SUM of LONG column %s could overflow int64"
    if f in (Q.MIN, Q.MAX) and null_handling and col.is_fp and col.has("nan"):
        return False                  # the reference is order dependent there (fuzz_cases' docstring)
    if f == Q.MAX and col.is_dict and col.is_fp and col.has("nan"):
        return False                  # "group-by MAX of dictionary column %s whose dictionary holds NaN": tests/test_gpu_fuzz_typed.py keeps that decline
    return True


def _derive_one(rng, counter, seg, fq, base_index, family, keys, variant):
    cols = seg.cols
    nh = fq.null_handling
    candidates = {raw: [i for i, c in enumerate(cols) if c.is_dict != raw and not (nh and c.nulls is not None)] for raw in (False, True)}
    encodings = [raw for raw in (False, True) if candidates[raw]]
    if not encodings:
        return None
    raw = encodings[int(rng.integers(0, len(encodings)))]
    pool = candidates[raw]
    chosen = [pool[i] for i in rng.permutation(len(pool))[: int(rng.integers(1, MAX_VALUE_COLUMNS + 1))]]
    aggs = [(family, int(c)) for c in chosen]
    extras = []
    if rng.integers(0, 2):
        agg_cols = []
        for f, c in fq.aggs:
            if not _extra_ok(seg, f, c, bool(keys), nh):
                continue
            if c >= 0 and f != Q.COUNT and c not in agg_cols:
                if not keys and len(agg_cols) >= F.MAX_AGG_COLUMNS:
                    continue
                agg_cols.append(c)
            extras.append((f, c))
    if extras:
        aggs = aggs + extras
        aggs = [aggs[i] for i in rng.permutation(len(aggs))]
    elif rng.integers(0, 2):
        aggs = aggs + [(Q.COUNT, -1)]
    valid = fmt = None
    if rng.integers(0, 3) == 0 and len(fq.leaves()) < F.MAX_LEAVES:
        valid = D.random_mask(rng, seg.n, float(rng.choice(VALID_DENSITIES)))
        fmt = ("words", "roaring")[next(counter) % 2]
    return ValueQuery(base_index, family, raw, aggs, fq.tree, list(keys), nh, fq.limit if keys else 0, valid, fmt, variant)


def derive(seg, fq, rng, counter=None, base_index=-1):
    """Zero or more value queries of one base FuzzQuery."""
    counter = itertools.count() if counter is None else counter
    if not eligible(seg, fq):
        return []
    out = []
    keys = repaired_keys(seg, fq)
    for family in VALUE_FUNCTIONS:
        out.append(_derive_one(rng, counter, seg, fq, base_index, family, keys, "base"))
    if not fq.group_by:
        small = [i for i, c in enumerate(seg.cols) if c.is_dict and c.cardinality <= SMALL_KEY and not (fq.null_handling and c.nulls is not None)]
        if small and rng.integers(0, 2):
            key = [small[int(rng.integers(0, len(small)))]]
            for family in VALUE_FUNCTIONS:
                out.append(_derive_one(rng, counter, seg, fq, base_index, family, key, "small-key"))
    return [v for v in out if v is not None]


def make_value_queries(seg, queries):
    """Every derived query of a fuzz segment, in base-query order."""
    rng = np.random.default_rng([seg.seed, F.SEED_BASE, SALT])
    counter = itertools.count()
    out = []
    for bi, fq in enumerate(queries):
        out += derive(seg, fq, rng, counter, bi)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the exact model
# ------------------------------------------------------------------------------------------------------------------------------------
def model_mask(seg, vq):
    mask = F.filter_mask(seg, vq.companion)
    return mask if vq.valid is None else mask & vq.valid


def from_dictionary(seg, vq):
    """AggregationPlanNode.java:98-115 with DISTINCTCOUNT among DICTIONARY_BASED_FUNCTIONS: NonScanBasedAggregationOperator answers when the
    filter matches every doc, no aggregation argument -- COUNT(column)'s included (hasNullValues :130-153) -- has null values under null
    handling, and every function is COUNT or has a dictionary to read (DISTINCTCOUNT, MIN, MAX on dictionary columns)."""
    if vq.family != Q.DISTINCTCOUNT or vq.raw or vq.group_by or vq.valid is not None:
        return False
    t = vq.tree
    if not (t is None or (t[0] == "leaf" and ((t[1].kind == "match_all" and not t[1].exclusive) or (t[1].kind == "match_none" and t[1].exclusive)))):
        return False
    if vq.null_handling and any(c >= 0 and seg.cols[c].nulls is not None for _, c in vq.aggs):
        return False
    return all(f == Q.COUNT or f == Q.DISTINCTCOUNT or (f in (Q.MIN, Q.MAX) and seg.cols[c].is_dict) for f, c in vq.aggs)


class ValueModel:
    """`lists`: {aggregation index: (want, docs)} or -- GROUP BY -- {key identity tuple: {aggregation index: (want, docs)}}; want: sorted
    dictIds / (dictIds, counts) / (value bits, counts); docs: the docs that reached the aggregation."""

    def __init__(self):
        self.mask, self.lists, self.whole_dictionary = None, {}, False


def _one_list(col, docs, family, raw):
    if raw:
        return RV.runs_of(col.values[docs])
    if family == Q.DISTINCTCOUNT:
        return np.unique(col.ids[docs]).astype(np.int32)
    d, n = np.unique(col.ids[docs], return_counts=True)
    return d.astype(np.int32), n.astype(np.uint32)


def model(seg, vq, mask=None):
    out = ValueModel()
    out.mask = model_mask(seg, vq) if mask is None else mask
    docs = np.flatnonzero(out.mask)
    out.whole_dictionary = from_dictionary(seg, vq)
    if out.whole_dictionary:
        out.lists = {a: (np.arange(seg.cols[vq.aggs[a][1]].cardinality, dtype=np.int32), docs) for a in vq.value_positions}
        return out
    per = lambda d: {a: (_one_list(seg.cols[vq.aggs[a][1]], d, vq.family, vq.raw), d) for a in vq.value_positions}
    if not vq.group_by:
        out.lists = per(docs)
        return out
    # identity tuples as F.expected's (no key here is nullable under null handling: no null digit)
    ident = [F.key_identity(seg.cols[g].values)[docs] for g in vq.group_by]
    rows = np.stack(ident, axis=1) if len(docs) else np.zeros((0, len(ident)), np.int64)
    uniq, inverse = np.unique(rows, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    order = np.argsort(inverse, kind="stable")
    bounds = np.searchsorted(inverse[order], np.arange(len(uniq) + 1))
    for u in range(len(uniq)):
        out.lists[tuple(int(x) for x in uniq[u])] = per(docs[order[bounds[u]: bounds[u + 1]]])
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# a device Result against the model
# ------------------------------------------------------------------------------------------------------------------------------------
def check_value(v, want, family, raw, where):
    """One AggValue of a value function: the list element for element; count = the list's length (PERCENTILE) or its distinct values
    (DISTINCTCOUNT); sum 0, min +inf, max -inf; no other form beside it (assert_sets_equal / assert_counts_equal / assert_lists_equal)."""
    if raw:
        assert v.value_counts is not None and v.dict_ids is None and v.dict_id_counts is None, "%s: no value list came back" % where
        bits, counts = v.value_counts
        assert bits.dtype == np.int64 and counts.dtype == np.uint32
        assert np.array_equal(bits, want[0]), "%s: values differ (%d runs, model %d)" % (where, len(bits), len(want[0]))
        assert np.array_equal(counts, want[1]), "%s: counts differ" % where
        want_count = int(want[1].astype(np.int64).sum()) if family == Q.PERCENTILE else len(want[0])
    elif family == Q.DISTINCTCOUNT:
        assert v.dict_ids is not None and v.dict_id_counts is None and v.value_counts is None, "%s: no set came back" % where
        assert np.array_equal(v.dict_ids, want), "%s: set differs (%d dictIds, model %d)" % (where, len(v.dict_ids), len(want))
        want_count = len(want)
    else:
        assert v.dict_id_counts is not None and v.dict_ids is None and v.value_counts is None, "%s: no list came back" % where
        ids, counts = v.dict_id_counts
        assert ids.dtype == np.int32 and counts.dtype == np.uint32
        assert np.array_equal(ids, want[0]), "%s: dictIds differ (%d, model %d)" % (where, len(ids), len(want[0]))
        assert np.array_equal(counts, want[1]), "%s: counts differ" % where
        want_count = int(want[1].astype(np.int64).sum())
    assert v.count == want_count, "%s: count %d, model %d" % (where, v.count, want_count)
    assert v.sum == 0.0 and v.sum_i64 == 0 and not v.sum_exact and v.min == float("inf") and v.max == float("-inf"), (where, v)


def percentile_of(col, v, raw, p):
    """The final result from what came back: the dictionary's / the bits' doubles through percentile_cases.percentile_of_counts."""
    if raw:
        bits, counts = v.value_counts
        return P.percentile_of_counts(RV.double_of_bits(bits, col.is_fp), counts, p)
    ids, counts = v.dict_id_counts
    return P.percentile_of_counts(np.asarray(col.dict_values)[ids.astype(np.int64)].astype(np.float64), counts, p)


def model_percentile(col, docs, p):
    """np.sort(doubles of the docs)[percentile_index] with the sort in Double.compare's order (the order image), -inf on empty."""
    d = col.doubles()[docs]
    if len(d) == 0:
        return float("-inf")
    return float(d[np.argsort(RV.order_image(d), kind="stable")][P.percentile_index(len(d), p)])


def result_rows(seg, vq, result):
    """{key identity tuple: [AggValue]} of a grouped result (F.result_keys), or {(): aggregations}."""
    return F.result_keys(seg, vq.companion, result) if vq.group_by else {(): result.aggregations}


def check_values(seg, vq, result, m, where=""):
    """Every value aggregation of the result against the model: lists, counts, the group set, and PERCENTILE's final answers."""
    rows = result_rows(seg, vq, result)
    lists = m.lists if vq.group_by else {(): m.lists}
    assert sorted(rows, key=repr) == sorted(lists, key=repr), "%s: groups differ (%d rows, model %d)" % (where, len(rows), len(lists))
    for key, per in lists.items():
        for a, (want, docs) in per.items():
            at = "%s group %r agg %d" % (where, key, a)
            v = rows[key][a]
            check_value(v, want, vq.family, vq.raw, at)
            if vq.family == Q.PERCENTILE:
                col = seg.cols[vq.aggs[a][1]]
                for p in PERCENTILES:
                    got_p, want_p = percentile_of(col, v, vq.raw, p), model_percentile(col, docs, p)
                    assert got_p == want_p or (np.isnan(got_p) and np.isnan(want_p)), "%s: PERCENTILE%d %r, model %r" % (at, p, got_p, want_p)
        for a, (f, _) in enumerate(vq.aggs):
            if f not in VALUE_FUNCTIONS:
                v = rows[key][a]
                assert v.dict_ids is None and v.dict_id_counts is None and v.value_counts is None, "%s: a list beside an ordinary function" % where


def post_filter_entries(seg, vq, m):
    """numEntriesScannedPostFilter: numDocsScanned x the distinct columns the ORIGINAL query projects; 0 when the dictionaries answered."""
    spec = Q.QuerySpec(vq.aggs, group_by=vq.group_by, null_handling=vq.null_handling)
    return 0 if m.whole_dictionary else int(m.mask.sum()) * DC.projected_columns(spec)


def ordinary_view(vq, got, want, seg, m):
    """`got` as the companion query would have returned it: the statistic of the original query's projection checked here and replaced by
    the companion's, the value positions by the reference side's COUNT(*) -- what F.check_result and helpers.assert_results_equal compare."""
    assert got.stats[2] == post_filter_entries(seg, vq, m), "numEntriesScannedPostFilter %r, model %d" % (got.stats, post_filter_entries(seg, vq, m))
    view = copy.copy(got)
    view.stats = (got.stats[0], got.stats[1], want.stats[2], got.stats[3])
    view.functions = list(want.functions)
    pairs = [(got.aggregations, want.aggregations)] if not vq.group_by else [(got.groups[g], want.groups[g]) for g in got.groups if g in want.groups]
    replaced = []
    for mine, theirs in pairs:
        row = list(mine)
        for a in vq.value_positions:
            if mine and theirs:
                row[a] = theirs[a]
        replaced.append(row)
    if not vq.group_by:
        view.aggregations = replaced[0]
    else:
        view.groups = dict(got.groups)
        for g, row in zip([g for g in got.groups if g in want.groups], replaced):
            view.groups[g] = row
    return view


def same_value_lists(one, other, vq):
    """Two device results of one query hold identical lists and statistics (raw_value_cases.same_lists and its dictionary equivalents)."""
    assert one.stats == other.stats and one.filter_entries_exact == other.filter_entries_exact
    assert one.group_keys == other.group_keys and sorted(one.groups, key=repr) == sorted(other.groups, key=repr)
    rows = [(one.aggregations, other.aggregations)] if not vq.group_by else [(one.groups[g], other.groups[g]) for g in one.groups]
    for ra, rb in rows:
        for a in vq.value_positions:
            assert ra[a].count == rb[a].count
            for field in ("dict_ids", "dict_id_counts", "value_counts"):
                x, y = getattr(ra[a], field), getattr(rb[a], field)
                assert (x is None) == (y is None)
                if x is not None:
                    x, y = (x, y) if isinstance(x, tuple) else ((x,), (y,))
                    assert all(np.array_equal(p, q) for p, q in zip(x, y)), "the %s of aggregation %d differ" % (field, a)
        same = lambda x, y: x == y or (x != x and y != y)
        for a in range(len(vq.aggs)):
            if a not in vq.value_positions:
                # every field, == or both NaN; a FLOAT / DOUBLE sum (sum_exact = 0) is added in no fixed order on the device: callers hold it to the model's bound
                assert ra[a].count == rb[a].count and ra[a].sum_i64 == rb[a].sum_i64 and ra[a].sum_exact == rb[a].sum_exact, "aggregation %d" % a
                assert same(ra[a].min, rb[a].min) and same(ra[a].max, rb[a].max), "aggregation %d: min / max differ" % a
                assert not ra[a].sum_exact or ra[a].sum == rb[a].sum, "aggregation %d: sums differ" % a


# ------------------------------------------------------------------------------------------------------------------------------------
# coverage
# ------------------------------------------------------------------------------------------------------------------------------------
def coverage(segments_and_queries):
    """What a seed set's derived queries exercise, as a Counter of labels (tests/test_fuzz_value_cases_cpu.py holds it to thresholds)."""
    from collections import Counter
    c = Counter()
    for seg, vqs in segments_and_queries:
        for vq in vqs:
            name = FAMILIES[vq.family]
            c["derived"] += 1
            c["function:" + name] += 1
            c["value_columns:%d" % len(vq.value_columns)] += 1
            c["grouped:%s" % ("yes" if vq.group_by else "no")] += 1
            c["grouped:" + name] += bool(vq.group_by)
            c["keys:%d" % len(vq.group_by)] += 1
            c["variant:" + vq.variant] += 1
            c["pass_alone:%s" % ("yes" if (vq.counts_only and not vq.group_by) else "no")] += 1
            c["pass_alone:" + name + (":raw" if vq.raw else ":dict")] += vq.counts_only and not vq.group_by
            c["null_handling:%s" % ("on" if vq.null_handling else "off")] += 1
            c["doc_set:%s" % (vq.valid_format or "none")] += 1
            if vq.valid is not None:
                c["doc_set_density:%s" % ("empty" if not vq.valid.any() else ("full" if vq.valid.all() else "partial"))] += 1
            c["whole_dictionary"] += from_dictionary(seg, vq)
            for col in vq.value_columns:
                cc = seg.cols[col]
                c["encoding:" + cc.kind] += 1
                c["encoding:%s:%s" % (name, cc.kind)] += 1
                for what in ("nan", "inf", "zero"):
                    c["value_has:" + what] += cc.is_fp and cc.has(what)
            for g in vq.group_by:
                c["key_scale:" + seg.cols[g].key_scale()[0]] += 1
            leaves = list({id(x): x for x in vq.leaves()}.values())
            c["leaves:%s" % ("0" if not leaves else ("1" if len(vq.leaves()) == 1 else ("2" if len(vq.leaves()) == 2 else "3+")))] += 1
            c["shared_pred"] += len(vq.leaves()) != len(leaves)
            for leaf in leaves:
                c["leaf:" + leaf.kind] += 1
            c["dict_set_leaves:2+"] += sum(x.kind == "dict_set" for x in leaves) >= 2
            c["inverted_leaf"] += any(x.kind in ("inverted_range", "inverted_set") for x in leaves)
            c["is_null_under_null_handling"] += vq.null_handling and any(x.kind == "is_null" for x in leaves)
            c["extras"] += any(f not in VALUE_FUNCTIONS and not (f == Q.COUNT and col < 0) for f, col in vq.aggs)
    return c
