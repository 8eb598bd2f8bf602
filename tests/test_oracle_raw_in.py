"""The yardstick of tests/test_gpu_raw_in.py, pinned: the oracle over the TWIN segment (filtered columns dictionary-encoded, the list a scan
PG_PRED_DICT_SET; tests/raw_in_cases.py) against numpy -- all four column types, IN and NOT IN, alone and under AND / OR / NOT, the
aggregated values and all four statistics."""
import numpy as np

import helpers as H
import raw_in_cases as R
from oracle import oracle
from pinot_amd import query as Q

N = 50_003


def test_one_leaf_against_numpy():
    _, twin, vals = R.segments(N, seed=1)
    _, pools = R.column_values(N, seed=1)
    rng = np.random.default_rng(1)
    for column in range(4):
        for values in R.value_lists(pools, column, rng):
            for exclusive in (False, True):
                mask = R.member_mask(vals, column, values) != exclusive
                got = oracle.execute(twin, Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, R.AI), (Q.MIN, R.AI), (Q.MAX, R.AL), (Q.SUM, R.DV)],
                                                       filter=Q.leaf(R.twin_pred(twin, column, values, exclusive))))
                m = int(mask.sum())
                assert 0 < m < N
                assert got.aggregations[0].count == m
                assert got.aggregations[1].sum_i64 == int(vals["ai"][mask].astype(np.int64).sum())
                assert got.aggregations[2].min == float(vals["ai"][mask].min())
                assert got.aggregations[3].max == float(vals["al"][mask].max())
                assert got.aggregations[4].sum_i64 == int(vals["dv"][mask].astype(np.int64).sum())
                # a ScanBasedFilterOperator looks at every doc once; three projected columns
                assert got.stats == (m, N, 3 * m, N) and got.filter_entries_exact


def test_compositions_against_numpy():
    _, twin, vals = R.segments(N, seed=2, distinct=300)
    _, pools = R.column_values(N, seed=2, distinct=300)
    rng = np.random.default_rng(2)
    a = pools["ri"][rng.choice(len(pools["ri"]), 120, replace=False)].tolist()
    d = pools["rd"][rng.choice(len(pools["rd"]), 100, replace=False)].tolist()
    ma, md = R.member_mask(vals, 0, a), R.member_mask(vals, 3, d)
    mf = (vals["f"] >= 20) & (vals["f"] < 180)
    la, ld, lf = Q.leaf(R.twin_pred(twin, 0, a)), Q.leaf(R.twin_pred(twin, 3, d)), Q.leaf(Q.Pred.dict_range(R.F, 20, 180))
    for flt, mask, entries in ((Q.and_(la, lf), ma & mf, H.and_leapfrog_entries([ma, mf])), (Q.and_(la, ld), ma & md, H.and_leapfrog_entries([ma, md])),
                               (Q.or_(ld, lf), md | mf, 2 * N), (Q.not_(la), ~ma, N), (Q.and_(lf, Q.not_(la)), mf & ~ma, None)):      # (a NOT child re-scans: its count is the iterator model's own, tests/test_filter_stats*.py)
        got = oracle.execute(twin, Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, R.AI)], filter=flt))
        assert got.aggregations[0].count == int(mask.sum())
        assert got.aggregations[1].sum_i64 == int(vals["ai"][mask].astype(np.int64).sum())
        assert got.filter_entries_exact and (entries is None or got.stats[1] == entries), (got.stats, entries)


def test_the_oracles_own_raw_set_leaf_against_numpy_and_the_twin():
    """PG_PRED_RAW_SET in the oracle itself (Int / Long / Float / DoubleRawValueBasedInPredicateEvaluator.applySV,
    InPredicateEvaluatorFactory.java:215-300) over the RAW segment: the same docs as numpy's membership and the same result, bitmap and
    statistics as the twin yardstick above -- a scan leaf's accounting does not depend on how its column is encoded."""
    raw, twin, vals = R.segments(N, seed=1)
    _, pools = R.column_values(N, seed=1)
    rng = np.random.default_rng(1)
    aggs = [(Q.COUNT, -1), (Q.SUM, R.AI), (Q.MIN, R.AI), (Q.MAX, R.AL), (Q.SUM, R.DV)]
    for column in range(4):
        for values in R.value_lists(pools, column, rng):
            for exclusive in (False, True):
                mask = R.member_mask(vals, column, values) != exclusive
                spec = Q.QuerySpec(aggs, filter=Q.leaf(R.raw_pred(column, values, exclusive)))
                got = oracle.execute(raw, spec)
                H.assert_results_equal(got, oracle.execute(twin, Q.QuerySpec(aggs, filter=Q.leaf(R.twin_pred(twin, column, values, exclusive)))))
                assert got.aggregations[0].count == int(mask.sum()) and got.stats == (int(mask.sum()), N, 3 * int(mask.sum()), N) and got.filter_entries_exact
                words, card = oracle.filter_bitmap(raw, spec)
                assert card == int(mask.sum()) and np.array_equal(np.unpackbits(words.view(np.uint8), bitorder="little")[:N].astype(bool), mask)
    # members that can never match: a long outside int32 on the INT column, a double that is not a float on the FLOAT column; the empty list
    some_int, some_float = int(vals["ri"][7]), float(vals["rf"][7])
    for column, values, hits in ((0, [2 ** 40 + some_int, some_int], vals["ri"] == some_int), (2, [0.1, some_float], vals["rf"] == np.float32(some_float)),
                                 (2, [float(np.float32(0.1))], vals["rf"] == np.float32(0.1)), (1, [], np.zeros(N, bool))):
        for exclusive in (False, True):
            got = oracle.execute(raw, Q.QuerySpec([(Q.COUNT, -1)], filter=Q.leaf(R.raw_pred(column, values, exclusive))))
            assert got.aggregations[0].count == int((hits != exclusive).sum()) and got.stats[1] == N
    assert int((vals["rf"] == np.float32(0.1)).sum()) > 0 and int((vals["ri"] == some_int).sum()) > 0


def test_the_oracles_raw_set_leaf_in_compositions_and_under_null_handling():
    rng = np.random.default_rng(2)
    nulls = rng.random(N) < 0.2
    raw, twin, vals = R.segments(N, seed=2, null_mask=nulls, distinct=300)
    _, pools = R.column_values(N, seed=2, distinct=300)
    a = pools["ri"][rng.choice(len(pools["ri"]), 120, replace=False)].tolist()
    d = pools["rd"][rng.choice(len(pools["rd"]), 100, replace=False)].tolist()

    def trees(seg_is_raw):
        la = Q.leaf(R.raw_pred(0, a) if seg_is_raw else R.twin_pred(twin, 0, a))
        ld = Q.leaf(R.raw_pred(3, d, True) if seg_is_raw else R.twin_pred(twin, 3, d, True))
        lf = Q.leaf(Q.Pred.dict_range(R.F, 20, 180))
        return [Q.and_(la, lf), Q.and_(la, ld), Q.or_(ld, lf), Q.not_(la), Q.and_(lf, Q.not_(la)), Q.or_(Q.and_(la, ld), Q.not_(lf))]
    for null_handling in (False, True):
        for group_by in ([], [R.GK]):
            for on_raw, on_twin in zip(trees(True), trees(False)):
                kw = dict(group_by=group_by, null_handling=null_handling)
                got = oracle.execute(raw, Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, R.AI), (Q.COUNT, 0)], filter=on_raw, **kw))
                H.assert_results_equal(got, oracle.execute(twin, Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, R.AI), (Q.COUNT, 0)], filter=on_twin, **kw)))
    # under null handling the leaf's trues leave the column's null docs out, and NOT does not bring them back (BaseFilterOperator.java:85-113)
    ma = R.member_mask(vals, 0, a)
    for tree, mask in ((Q.leaf(R.raw_pred(0, a)), ma & ~nulls), (Q.not_(Q.leaf(R.raw_pred(0, a))), ~ma & ~nulls), (Q.leaf(R.raw_pred(0, a, True)), ~ma & ~nulls)):
        got = oracle.execute(raw, Q.QuerySpec([(Q.COUNT, -1)], filter=tree, null_handling=True))
        assert got.aggregations[0].count == int(mask.sum())
