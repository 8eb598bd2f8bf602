"""VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP on the device (PG_AGG_VARIANCE, pg_result_moments): the VarianceTuple (count, sum, m2) of every
value family, raw and dictionary-encoded, against the exact model of tests/moments_cases.py over the docs oracle.filter_bitmap matches.

The bound is moments_cases.tol: derived from the two-run scheme's arithmetic, not from what the kernels return.  `count` is held to COUNT(*),
`sum` bit for bit to a PG_AGG_SUM of the same column in the same query."""
import math

import numpy as np
import pytest

import moments_cases as M
from oracle import oracle
from pinot_amd import query as Q
from pinot_amd import segment as S

pytestmark = pytest.mark.gpu

SCAN, GROUP = "scan_moments_kernel", "group_moments_kernel"
# four VARIANCE columns per query (kMaxAggCols): the families in three helpings
HELPINGS = [list(range(0, 4)), list(range(4, 8)), list(range(8, len(M.VALUE_COLUMNS)))]


def aggs_of(columns):
    """VARIANCE and SUM of every column, COUNT(*) last."""
    return [(Q.VARIANCE, c) for c in columns] + [(Q.SUM, c) for c in columns] + [(Q.COUNT, -1)]


def check(g, seg, spec, where, kernel=None):
    got = g.execute(spec)
    want = M.assert_moments(got, seg, spec, where=where)
    other = oracle.execute(seg, Q.QuerySpec([(Q.COUNT, -1)], filter=spec.filter, group_by=spec.group_by))
    count_at = len(spec.aggregations) - 1
    if spec.group_by:
        assert all(v[count_at].count == other.groups[gid][0].count == want[gid][0][0] for gid, v in got.groups.items()), where
    else:
        assert got.aggregations[count_at].count == other.aggregations[0].count == want[0][0], where
        if kernel is not None and want[0][0] > 0:
            assert got.dominant_kernel in (kernel, g.execute(M.without_variance(spec)).dominant_kernel), (where, got.dominant_kernel)
    return got


@pytest.mark.parametrize("raw", [True, False], ids=["raw", "dict"])
@pytest.mark.parametrize("num_docs,one_cu", [(n, False) for n in M.SIZES] + [(M.BIG, True)])
def test_every_family_behind_every_filter(engine, monkeypatch, num_docs, one_cu, raw):
    if one_cu:
        monkeypatch.setenv("PINOT_GPU_TEST_CUS", "1")                   # a grid sized for one CU: every wave takes several tiles
    seg = M.build_segment(S, num_docs, raw)
    n = num_docs
    tag = "%s n=%d%s" % ("raw" if raw else "dict", n, " one CU" if one_cu else "")
    f_lt = lambda t: Q.leaf(Q.Pred.dict_range(M.C_FILTER, 0, t))
    in_list = Q.leaf(Q.Pred.dict_set(M.C_SET, list(range(0, 300, 7)), 300))
    with engine.open(seg) as g:
        for columns in HELPINGS:
            at = "%s cols %s" % (tag, columns)
            got = check(g, seg, Q.QuerySpec(aggs_of(columns)), at + " no filter", kernel=SCAN)
            # there is no metadata fast path: the columns are scanned, and counted as projected
            assert got.stats == (n, 0, len(columns) * n, n), got.stats
            check(g, seg, Q.QuerySpec(aggs_of(columns), filter=f_lt(500)), at + " range leaf", kernel=SCAN)
            check(g, seg, Q.QuerySpec(aggs_of(columns), filter=in_list), at + " IN leaf (staged set)", kernel=SCAN)
            got = check(g, seg, Q.QuerySpec(aggs_of(columns), filter=Q.leaf(Q.Pred.match_none())), at + " no match")
            assert all(v.moments == (0, 0.0, 0.0) for v in got.aggregations[:len(columns)])
            assert got.dominant_kernel not in (SCAN, GROUP)              # count 0: the pass is not launched
            check(g, seg, Q.QuerySpec(aggs_of(columns), group_by=[M.C_K1]), at + " one key")
            got = check(g, seg, Q.QuerySpec(aggs_of(columns), filter=f_lt(700), group_by=[M.C_K1, M.C_K2]), at + " two keys behind a filter")
            assert got.group_id_upper_bound == 35


def test_the_scalar_pass_returns_the_same_bits_twice(engine):
    seg = M.build_segment(S, M.BIG, raw=True)
    spec = Q.QuerySpec(aggs_of(HELPINGS[0]), filter=Q.leaf(Q.Pred.dict_range(M.C_FILTER, 0, 500)))
    with engine.open(seg) as g:
        first, second = g.execute(spec), g.execute(spec)
    assert first.dominant_kernel in (SCAN, "scan_private_typed_kernel", "scan_agg_kernel"), first.dominant_kernel
    for a in range(4):
        assert np.float64(first.aggregations[a].moments[2]).tobytes() == np.float64(second.aggregations[a].moments[2]).tobytes(), a


def test_the_pass_kernels_are_the_ones_that_run(engine):
    """The pass reports its own kernel when it is the longer of the two runs: on a segment whose ordinary query is COUNT + AVG of one narrow
    column, the pass (which converts every value to double) is not the shorter one by much either way, so the name is one of exactly two."""
    seg = M.build_segment(S, M.BIG, raw=False)
    with engine.open(seg) as g:
        for group_by, kernel in (([], SCAN), ([M.C_K1], GROUP)):
            spec = Q.QuerySpec([(Q.VARIANCE, 0)], group_by=group_by)
            ordinary = g.execute(Q.QuerySpec([(Q.AVG, 0)], group_by=group_by)).dominant_kernel
            assert ordinary not in (kernel, ""), ordinary
            assert g.execute(spec).dominant_kernel in (kernel, ordinary)


def test_a_constant_column_has_a_standard_deviation(engine):
    for raw in (True, False):
        seg = M.build_segment(S, M.BIG, raw)
        columns = [M.VALUE_COLUMNS.index("int_const7"), M.VALUE_COLUMNS.index("double_const01")]
        with engine.open(seg) as g:
            got = g.execute(Q.QuerySpec(aggs_of(columns), filter=Q.leaf(Q.Pred.dict_range(M.C_FILTER, 0, 900))))
        for a in range(2):
            t = got.aggregations[a].moments
            for kind in ("stddevpop", "stddevsamp"):
                value = M.final(kind, t)
                assert not math.isnan(value) and value >= 0.0, (raw, a, kind, t)
        assert got.aggregations[0].moments[2] == 0.0                      # an INT constant: the pivot is the value itself
