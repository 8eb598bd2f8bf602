"""Shared builders and the exact model of the DISTINCTCOUNT tests (tests/test_distinct_cpu.py, tests/test_gpu_distinct.py,
tools/kernel_coverage.py, tools/bench_variants.py).

The model is not the oracle (which knows nothing of DISTINCTCOUNT): per DISTINCTCOUNT aggregation -- and per group -- it is
`np.unique(dictIds[matching])`, with `matching` from `oracle.filter_bitmap` and the dictIds read back from the column's forward index
(`oracle.read_dict_ids`).  Everything is compared exactly, set element for set element.
"""
import numpy as np

from oracle import oracle
from pinot_amd import query as Q

# InterSegmentAggregationSingleValueQueriesTest.testDistinctCount (:235-258) over tests/golden/test_data_sv.npz: v1 = DISTINCTCOUNT(column1),
# v2 = DISTINCTCOUNT(column3); per-segment statistics (numDocsScanned, numEntriesScannedInFilter, numEntriesScannedPostFilter, numTotalDocs).
GOLDEN_GROUP_KEY = 296467636          # the column9 value of the `ORDER BY v1 DESC, v2 DESC LIMIT 1` row
GOLDEN_ROWS = {
    "plain": {"v1": 6582, "v2": 21910, "stats": (30000, 0, 0, 30000)},
    "filter": {"v1": 1872, "v2": 4556, "stats": (6129, 63064, 12258, 30000)},
    "group": {"v1": 3495, "v2": 11961, "stats": (30000, 0, 90000, 30000)},
    "filter+group": {"v1": 1272, "v2": 3289, "stats": (6129, 63064, 18387, 30000)},
}


def dict_ids_of(seg, column):
    """Every doc's dictId of a dictionary column, decoded from the forward index the engine is handed."""
    c = seg.columns[column]
    assert c.dictionary is not None, "DISTINCTCOUNT is defined on dictionary columns here"
    cache = seg.__dict__.setdefault("_distinct_dict_ids", {})
    if column not in cache:
        cache[column] = oracle.read_dict_ids(c.fwd, c.bits, seg.num_docs, np.arange(seg.num_docs, dtype=np.int32))
    return cache[column]


def matching_docs(seg, spec):
    """bool[num_docs]: the docs the spec's filter matches, from the oracle."""
    only_filter = Q.QuerySpec([], filter=spec.filter, null_handling=spec.null_handling)
    words, card = oracle.filter_bitmap(seg, only_filter)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:seg.num_docs].astype(bool)
    assert int(bits.sum()) == card
    return bits


def group_ids_of(seg, spec, key_values=None):
    """Every doc's raw group id: sum digit_j * prod_{k<j} cardinality_k (DictionaryBasedGroupKeyGenerator.java:437-445).
    key_values: {column: (int array of per-doc values, base, cardinality)} for raw key columns (digit = value - base)."""
    gid = np.zeros(seg.num_docs, dtype=np.int64)
    mult = 1
    for c in spec.group_by:
        if key_values and c in key_values:
            values, base, card = key_values[c]
            digit = np.asarray(values, dtype=np.int64) - base
        else:
            digit, card = dict_ids_of(seg, c).astype(np.int64), seg.columns[c].cardinality
        gid += digit * mult
        mult *= card
    return gid


def model(seg, spec, key_values=None):
    """{aggregation index: sorted dictIds} of every DISTINCTCOUNT aggregation, or -- GROUP BY -- {raw group id: {aggregation index:
    sorted dictIds}} over the groups that hold a matching doc."""
    match = matching_docs(seg, spec)
    distinct = [(a, c) for a, (f, c) in enumerate(spec.aggregations) if f == Q.DISTINCTCOUNT]
    if not spec.group_by:
        return {a: np.unique(dict_ids_of(seg, c)[match]).astype(np.int32) for a, c in distinct}
    gid = group_ids_of(seg, spec, key_values)[match]
    order = np.argsort(gid, kind="stable")
    bounds = np.flatnonzero(np.diff(gid[order])) + 1
    matched = {c: dict_ids_of(seg, c)[match] for _, c in distinct}
    out = {}
    for rows in np.split(order, bounds) if gid.shape[0] else []:
        out[int(gid[rows[0]])] = {a: np.unique(matched[c][rows]).astype(np.int32) for a, c in distinct}
    return out


def without_distinct(spec):
    """The spec the oracle can run: every DISTINCTCOUNT turned into COUNT(*) (same positions, same filter, keys and flags)."""
    aggs = [((Q.COUNT, -1) if f == Q.DISTINCTCOUNT else (f, c)) for f, c in spec.aggregations]
    return Q.QuerySpec(aggs, filter=spec.filter, group_by=spec.group_by, null_handling=spec.null_handling, num_groups_limit=spec.num_groups_limit,
                       stats_upper_bound_ok=spec.stats_upper_bound_ok)


def projected_columns(spec):
    """Distinct columns the query projects: numEntriesScannedPostFilter = numDocsScanned x this."""
    cols = set(spec.group_by)
    for f, c in spec.aggregations:
        if f != Q.COUNT or (spec.null_handling and c >= 0):
            cols.add(c)
    return len(cols)


def assert_sets_equal(got, seg, spec, want=None, key_values=None, where=""):
    """The result's DISTINCTCOUNT fields against the model: count = |set|, sum 0, min +inf, max -inf, the set element for element."""
    want = model(seg, spec, key_values) if want is None else want

    def one(v, ids, at):
        assert v.dict_ids is not None, "%s %s: no set came back" % (where, at)
        assert np.array_equal(v.dict_ids, ids), "%s %s: set differs (%d dictIds, model %d)" % (where, at, len(v.dict_ids), len(ids))
        assert v.count == len(ids) and v.sum == 0.0 and v.sum_i64 == 0 and not v.sum_exact and v.min == float("inf") and v.max == float("-inf"), (where, at, v)

    if not spec.group_by:
        for a, ids in want.items():
            one(got.aggregations[a], ids, "agg %d" % a)
        return
    assert sorted(got.groups) == sorted(want), "%s: groups differ (%d, model %d)" % (where, len(got.groups), len(want))
    for gid, sets in want.items():
        for a, ids in sets.items():
            one(got.groups[gid][a], ids, "group %d agg %d" % (gid, a))


def assert_other_functions_equal(got, seg, spec):
    """Every function of the query that is not a DISTINCTCOUNT, and the statistics, against the unchanged oracle."""
    import helpers as H
    want = oracle.execute(seg, without_distinct(spec))
    for a, (f, _) in enumerate(spec.aggregations):
        if f == Q.DISTINCTCOUNT:
            continue
        if spec.group_by:
            assert sorted(got.groups) == sorted(want.groups), "group ids differ"
            for gid in want.groups:
                H.assert_agg_equal(got.groups[gid][a], want.groups[gid][a], f, "group %r agg %d" % (gid, a))
        else:
            H.assert_agg_equal(got.aggregations[a], want.aggregations[a], f, "agg %d" % a)
    assert got.stats[0] == want.stats[0] and got.stats[3] == want.stats[3], (got.stats, want.stats)
    assert got.stats[2] == got.stats[0] * projected_columns(spec), (got.stats, projected_columns(spec))
    if got.filter_entries_exact and want.filter_entries_exact:
        assert got.stats[1] == want.stats[1], (got.stats, want.stats)


def golden_spec(seg, filtered, grouped, filter_form="logical"):
    """One of testDistinctCount's four queries on H.golden_segment()."""
    import helpers as H
    flt = None
    if filtered:
        flt = {"logical": lambda: H.golden_filter(seg), "inverted": lambda: H.golden_filter(seg, inverted=True),
               "physical": lambda: H.golden_filter_physical(seg)}[filter_form]()
    ci = seg.column_index
    return Q.QuerySpec([(Q.DISTINCTCOUNT, ci("column1")), (Q.DISTINCTCOUNT, ci("column3"))], filter=flt, group_by=[ci("column9")] if grouped else [])


def golden_group_id(seg):
    c9 = seg.columns[seg.column_index("column9")]
    d = int(np.searchsorted(c9.dict_values, GOLDEN_GROUP_KEY))
    assert c9.value_of(d) == GOLDEN_GROUP_KEY
    return d


def synthetic_segment(S, name, num_docs, cardinalities, seed=5, last_present=True):
    """Dictionary columns of the given cardinalities over `num_docs` docs; with last_present every column's largest dictId occurs."""
    rng = np.random.default_rng(seed)
    cols = []
    for i, card in enumerate(cardinalities):
        ids = rng.integers(0, card, num_docs).astype(np.int32)
        if last_present and num_docs > 0:
            ids[int(rng.integers(0, num_docs))] = card - 1
        cols.append(S.Column.from_dict_ids("c%d" % i, (np.arange(card, dtype=np.int64) * 3 - card).astype(np.int32), ids))
    return S.SegmentData(name, num_docs, cols)
