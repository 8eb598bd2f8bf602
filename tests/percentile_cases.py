"""Shared builders and the exact model of the PERCENTILE tests (tests/test_percentile_cpu.py, tests/test_gpu_percentile.py,
tools/kernel_coverage.py, tools/bench_variants.py).

The model is not the oracle (which knows nothing of PERCENTILE): per PERCENTILE aggregation -- and per raw group id -- it is
`np.unique(dictIds[matching], return_counts=True)`, with `matching` from `oracle.filter_bitmap` and the dictIds read back from the column's
forward index (`oracle.read_dict_ids`), through the helpers of tests/distinct_cases.py.  Everything is compared exactly, pair for pair.
"""
import numpy as np

import distinct_cases as DC
from oracle import oracle
from pinot_amd import query as Q

matching_docs = DC.matching_docs
dict_ids_of = DC.dict_ids_of
group_ids_of = DC.group_ids_of
projected_columns = DC.projected_columns
synthetic_segment = DC.synthetic_segment
golden_group_id = DC.golden_group_id
GOLDEN_GROUP_KEY = DC.GOLDEN_GROUP_KEY

# InterSegmentAggregationSingleValueQueriesTest.testPercentile (:379-473) over tests/golden/test_data_sv.npz, four copies of the segment:
# v1 = PERCENTILE<p>(column1), v2 = PERCENTILE<p>(column3); the grouped rows are the `ORDER BY v1 DESC, v2 DESC LIMIT 1` row of GROUP BY column9.
# Per-segment statistics (numDocsScanned, numEntriesScannedInFilter, numEntriesScannedPostFilter, numTotalDocs).
GOLDEN_STATS = {
    "plain": (30000, 0, 60000, 30000),
    "filter": (6129, 63064, 12258, 30000),
    "group": (30000, 0, 90000, 30000),
    "filter+group": (6129, 63064, 18387, 30000),
}
GOLDEN_VALUES = {
    (50, "plain"): (1107310944.0, 1080136306.0), (50, "filter"): (1139674505.0, 505053732.0),
    (50, "group"): (2146791843.0, 1418523221.0), (50, "filter+group"): (2142595699.0, 334963174.0),
    (90, "plain"): (1943040511.0, 1936611145.0), (90, "filter"): (1936730975.0, 899534534.0),
    (90, "group"): (2146791843.0, 1418523221.0), (90, "filter+group"): (2142595699.0, 334963174.0),
    (95, "plain"): (2071559385.0, 2042409652.0), (95, "filter"): (2096857943.0, 947763150.0),
    (95, "group"): (2146791843.0, 1418523221.0), (95, "filter+group"): (2142595699.0, 334963174.0),
    (99, "plain"): (2139354437.0, 2125299552.0), (99, "filter"): (2146232405.0, 990669195.0),
    (99, "group"): (2146791843.0, 1418523221.0), (99, "filter+group"): (2146232405.0, 990259756.0),
}
GOLDEN_SHAPES = {"plain": (False, False), "filter": (True, False), "group": (False, True), "filter+group": (True, True)}


def percentile_index(size, p):
    """PercentileAggregationFunction.extractFinalResult (:155-172): `(int) ((long) size * percentile / 100)` -- long x double / 100, truncated;
    p == 100 is the last value."""
    if p == 100:
        return size - 1
    return int(float(size) * float(p) / 100.0)


def percentile_of_counts(values, counts, p):
    """The final result over ascending runs (value, count): the value at percentile_index of the expanded sorted list; -inf when it is empty."""
    counts = np.asarray(counts, dtype=np.int64)
    size = int(counts.sum())
    if size == 0:
        return float("-inf")
    at = int(np.searchsorted(np.cumsum(counts), percentile_index(size, p), side="right"))
    return float(np.asarray(values, dtype=np.float64)[at])


def model(seg, spec, key_values=None):
    """{aggregation index: (ascending dictIds int32, counts uint32)} of every PERCENTILE aggregation, or -- GROUP BY -- {raw group id: {...}}
    over the groups that hold a matching doc."""
    match = matching_docs(seg, spec)
    pct = [(a, c) for a, (f, c) in enumerate(spec.aggregations) if f == Q.PERCENTILE]

    def pairs(ids):
        d, n = np.unique(ids, return_counts=True)
        return d.astype(np.int32), n.astype(np.uint32)

    if not spec.group_by:
        return {a: pairs(dict_ids_of(seg, c)[match]) for a, c in pct}
    gid = group_ids_of(seg, spec, key_values)[match]
    order = np.argsort(gid, kind="stable")
    bounds = np.flatnonzero(np.diff(gid[order])) + 1
    matched = {c: dict_ids_of(seg, c)[match] for _, c in pct}
    out = {}
    for rows in np.split(order, bounds) if gid.shape[0] else []:
        out[int(gid[rows[0]])] = {a: pairs(matched[c][rows]) for a, c in pct}
    return out


def without_percentile(spec):
    """The spec the oracle can run: every PERCENTILE turned into COUNT(*) (same positions, same filter, keys and flags)."""
    aggs = [((Q.COUNT, -1) if f == Q.PERCENTILE else (f, c)) for f, c in spec.aggregations]
    return Q.QuerySpec(aggs, filter=spec.filter, group_by=spec.group_by, null_handling=spec.null_handling, num_groups_limit=spec.num_groups_limit,
                       stats_upper_bound_ok=spec.stats_upper_bound_ok)


def assert_counts_equal(got, seg, spec, want=None, key_values=None, where=""):
    """The result's PERCENTILE fields against the model: count = the docs aggregated, sum 0, min +inf, max -inf, the pairs one for one."""
    want = model(seg, spec, key_values) if want is None else want

    def one(v, pairs, at):
        assert v.dict_id_counts is not None, "%s %s: no list came back" % (where, at)
        ids, counts = v.dict_id_counts
        assert ids.dtype == np.int32 and counts.dtype == np.uint32
        assert np.array_equal(ids, pairs[0]), "%s %s: dictIds differ (%d, model %d)" % (where, at, len(ids), len(pairs[0]))
        assert np.array_equal(counts, pairs[1]), "%s %s: counts differ" % (where, at)
        assert v.count == int(pairs[1].astype(np.int64).sum()) and v.sum == 0.0 and v.sum_i64 == 0 and not v.sum_exact
        assert v.min == float("inf") and v.max == float("-inf"), (where, at, v.min, v.max)

    if not spec.group_by:
        for a, pairs in want.items():
            one(got.aggregations[a], pairs, "agg %d" % a)
        return
    assert sorted(got.groups) == sorted(want), "%s: groups differ (%d, model %d)" % (where, len(got.groups), len(want))
    for gid, lists in want.items():
        for a, pairs in lists.items():
            one(got.groups[gid][a], pairs, "group %d agg %d" % (gid, a))


def assert_other_functions_equal(got, seg, spec):
    """Every function of the query that is not a PERCENTILE, and the statistics, against the unchanged oracle."""
    import helpers as H
    want = oracle.execute(seg, without_percentile(spec))
    for a, (f, _) in enumerate(spec.aggregations):
        if f == Q.PERCENTILE:
            assert all(v[a].dict_ids is None for v in (got.groups.values() if spec.group_by else [got.aggregations]))
            continue
        if spec.group_by:
            assert sorted(got.groups) == sorted(want.groups), "group ids differ"
            for gid in want.groups:
                H.assert_agg_equal(got.groups[gid][a], want.groups[gid][a], f, "group %r agg %d" % (gid, a))
                assert got.groups[gid][a].dict_id_counts is None
        else:
            H.assert_agg_equal(got.aggregations[a], want.aggregations[a], f, "agg %d" % a)
            assert got.aggregations[a].dict_id_counts is None
    assert got.stats[0] == want.stats[0] and got.stats[3] == want.stats[3], (got.stats, want.stats)
    assert got.stats[2] == got.stats[0] * projected_columns(spec), (got.stats, projected_columns(spec))
    if got.filter_entries_exact and want.filter_entries_exact:
        assert got.stats[1] == want.stats[1], (got.stats, want.stats)


def golden_spec(seg, filtered, grouped, filter_form="logical"):
    """One of testPercentile's four query shapes on H.golden_segment() (the percentile is not part of the device query)."""
    import helpers as H
    flt = None
    if filtered:
        flt = {"logical": lambda: H.golden_filter(seg), "inverted": lambda: H.golden_filter(seg, inverted=True),
               "physical": lambda: H.golden_filter_physical(seg)}[filter_form]()
    ci = seg.column_index
    return Q.QuerySpec([(Q.PERCENTILE, ci("column1")), (Q.PERCENTILE, ci("column3"))], filter=flt, group_by=[ci("column9")] if grouped else [])


def values_of(seg, column, dict_ids):
    """The DOUBLE values behind dictIds of a numeric dictionary column (getDoubleValuesSV)."""
    return np.asarray(seg.columns[column].dict_values)[np.asarray(dict_ids, dtype=np.int64)].astype(np.float64)


def golden_finals(seg, lists, p, copies=4):
    """(v1, v2) of a golden row from the model's lists of one segment: `copies` identical segments multiply every count."""
    ci = seg.column_index
    out = []
    for a, name in ((0, "column1"), (1, "column3")):
        ids, counts = lists[a]
        out.append(percentile_of_counts(values_of(seg, ci(name), ids), counts.astype(np.int64) * copies, p))
    return tuple(out)
