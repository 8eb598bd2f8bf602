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
