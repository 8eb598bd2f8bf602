"""IN / NOT IN on raw INT / LONG / FLOAT / DOUBLE columns on the device (PG_PRED_RAW_SET), through the C ABI.  Expected values: the
oracle over the TWIN segment whose filtered columns are dictionary-encoded (tests/raw_in_cases.py; tests/test_oracle_raw_in.py pins that
yardstick to numpy), numpy for the bitmaps, the reference's goldens for the SQL."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import raw_in_cases as R
from oracle import oracle
from pinot_amd import _abi
from pinot_amd import host
from pinot_amd import query as Q
from test_oracle_range_not_queries import RANGE_KATS, fp_edge_segment, range_segment

pytestmark = pytest.mark.gpu

LEAN = "scan_raw_set_kernel"
SWITCH = "PINOT_GPU_SCAN_RAW_SET"


def agg_sets(column):
    """(aggregations, does scan_raw_set_kernel take them?)"""
    own = [(Q.MIN, column), (Q.MAX, column), (Q.COUNT, -1)] + ([(Q.SUM, column), (Q.AVG, column)] if column == 0 else [])
    return [([(Q.COUNT, -1)], True),
            ([(Q.SUM, R.AI), (Q.MIN, R.AI), (Q.MAX, R.AI), (Q.AVG, R.AI), (Q.COUNT, -1)], True),
            (own, column == 0),
            ([(Q.SUM, R.AL), (Q.MAX, R.AL)], False),
            ([(Q.SUM, R.AD), (Q.MIN, R.AD)], False),
            ([(Q.SUM, R.DV), (Q.MAX, R.DV), (Q.COUNT, -1)], False)]


def check_one_leaf(g, twin, column, values, exclusive, aggs, lean, switch_on):
    got = g.execute(Q.QuerySpec(aggs, filter=Q.leaf(R.raw_pred(column, values, exclusive))))
    want = oracle.execute(twin, Q.QuerySpec(aggs, filter=Q.leaf(R.twin_pred(twin, column, values, exclusive))))
    H.assert_results_equal(got, want, check_stats=True)
    assert got.filter_entries_exact and want.filter_entries_exact
    assert (got.dominant_kernel == LEAN) == (lean and switch_on), (got.dominant_kernel, column, len(values), exclusive, aggs)


@pytest.mark.parametrize("switch", [None, "0"])
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 70_001])
def test_one_leaf_every_type_list_size_and_aggregation(engine, switch, n):
    engine.reinit(**{SWITCH: switch})
    try:
        seg, twin, _ = R.segments(n, seed=n)
        _, pools = R.column_values(n, seed=n)
        rng = np.random.default_rng(n)
        with engine.open(seg) as g:
            for column in range(4):
                for values in R.value_lists(pools, column, rng):
                    for exclusive in (False, True):
                        for aggs, lean in agg_sets(column):
                            check_one_leaf(g, twin, column, values, exclusive, aggs, lean, switch is None)
    finally:
        engine.reinit(**{SWITCH: None})


@pytest.mark.parametrize("switch", [None, "0"])
@pytest.mark.parametrize("n,cus", [(300_017, "1"), (12_000_517, None)])
def test_one_leaf_many_tiles_per_wave_and_the_full_grid(engine, switch, n, cus):
    engine.reinit(**{SWITCH: switch, "PINOT_GPU_TEST_CUS": cus})
    try:
        seg, twin, _ = R.segments(n, seed=3)
        _, pools = R.column_values(n, seed=3)
        rng = np.random.default_rng(5)
        with engine.open(seg) as g:
            for column in range(4):
                lists = R.value_lists(pools, column, rng)
                for values in (lists[3], lists[4]):
                    for exclusive in (False, True):
                        for aggs, lean in agg_sets(column)[:3] + agg_sets(column)[5:]:
                            check_one_leaf(g, twin, column, values, exclusive, aggs, lean, switch is None)
    finally:
        engine.reinit(**{SWITCH: None, "PINOT_GPU_TEST_CUS": None})


def test_adversarial_lists_and_floating_point_edges(engine):
    """The lists the table builder is tested with on the CPU, as values of the columns' types; raw FLOAT / DOUBLE columns with NaN, signed
    zeros, infinities and subnormals (NaN values match nothing for IN and everything for NOT IN: no NaN can be listed)."""
    n = 20_011
    rng = np.random.default_rng(9)
    ints = np.array([-1, 0, -2 ** 31, 2 ** 31 - 1] + [i << 20 for i in range(-64, 64)], dtype=np.int64)
    longs = np.array([-1, 0, -2 ** 63, 2 ** 63 - 1] + [i << 40 for i in range(-64, 64)], dtype=np.int64)
    ri, rl = ints[rng.integers(0, len(ints), n)].astype(np.int32), longs[rng.integers(0, len(longs), n)]
    seg = R.S.SegmentData("adv", n, [R.S.Column.raw("ri", ri), R.S.Column.raw_typed("rl", rl)])
    with engine.open(seg) as g:
        for column, vals, lists in ((0, ri, [[-1, 0, -2 ** 31, 2 ** 31 - 1], [i << 20 for i in range(-64, 64, 2)], [2 ** 40, -2 ** 40, 5]]),
                                    (1, rl, [[-1, 0, -2 ** 63, 2 ** 63 - 1], [i << 40 for i in range(-64, 64, 2)], [12345]])):
            for values in lists:
                for exclusive in (False, True):
                    mask = np.isin(vals.astype(np.int64), np.array(values, dtype=np.int64)) != exclusive
                    got = g.execute(Q.QuerySpec([(Q.COUNT, -1)], filter=Q.leaf(Q.Pred.raw_set(column, values, exclusive))))
                    assert got.aggregations[0].count == int(mask.sum()) and got.stats[:2] == (int(mask.sum()), n) and got.filter_entries_exact
                    words, card = g.filter_bitmap(Q.QuerySpec([(Q.COUNT, -1)], filter=Q.leaf(Q.Pred.raw_set(column, values, exclusive))))
                    assert card == int(mask.sum()) and np.array_equal(np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool), mask)
    fseg, fv, dv = fp_edge_segment(3001)
    with engine.open(fseg) as g:
        for column, vals in ((0, fv), (1, dv)):
            finite = [v for v in np.unique(vals[np.isfinite(vals) & (vals != 0)]).tolist()]
            for values in ([np.inf], [-np.inf, np.inf], finite[:40], finite[::3] + [123.456]):
                listed = np.array(values, dtype=vals.dtype)
                for exclusive in (False, True):
                    mask = np.isin(vals, listed) != exclusive
                    got = g.execute(Q.QuerySpec([(Q.COUNT, -1)], filter=Q.leaf(Q.Pred.raw_set_f64(column, listed.tolist(), exclusive))))
                    assert got.aggregations[0].count == int(mask.sum()), (column, values, exclusive)


def composition_cases(twin_of):
    """(label, filter builder taking a leaf-maker) -- `mk(column, values, exclusive)` makes the raw or the twin leaf."""
    def cases(mk, lists):
        a, b, c = lists
        f_range = Q.leaf(Q.Pred.dict_range(R.F, 20, 180))
        return [
            ("set AND dictRange", Q.and_(Q.leaf(mk(0, a)), f_range)),
            ("dictRange AND set", Q.and_(f_range, Q.leaf(mk(1, b)))),
            ("set AND set", Q.and_(Q.leaf(mk(0, a)), Q.leaf(mk(3, c)))),
            ("set OR dictRange", Q.or_(Q.leaf(mk(2, c)), f_range)),
            ("NOT set", Q.not_(Q.leaf(mk(1, b)))),
            ("a AND NOT set", Q.and_(f_range, Q.not_(Q.leaf(mk(0, a))))),
            ("docRange AND set", Q.and_(Q.leaf(Q.Pred.doc_range(100, 40_000)), Q.leaf(mk(0, a, True)))),
            ("inverted AND set", Q.and_(Q.leaf(Q.Pred.dict_set(R.INV, [1, 3, 5], 12, inverted=True)), Q.leaf(mk(3, c)))),
        ]
    return cases


def test_compositions_with_exact_filter_statistics(engine):
    n = 50_003
    seg, twin, vals = R.segments(n, seed=21, distinct=300)
    _, pools = R.column_values(n, seed=21, distinct=300)
    rng = np.random.default_rng(2)
    lists = (pools["ri"][rng.choice(len(pools["ri"]), 120, replace=False)].tolist(), pools["rl"][rng.choice(len(pools["rl"]), 150, replace=False)].tolist(),
             pools["rd"][rng.choice(len(pools["rd"]), 100, replace=False)].tolist())
    flists = (lists[0], lists[1], pools["rf"][rng.choice(len(pools["rf"]), 100, replace=False)].tolist())
    build = composition_cases(None)
    raws = build(lambda c, v, e=False: R.raw_pred(c, flists[2] if c == 2 else v, e), lists)
    twins = build(lambda c, v, e=False: R.twin_pred(twin, c, flists[2] if c == 2 else v, e), lists)
    aggs = [(Q.COUNT, -1), (Q.SUM, R.DV), (Q.MAX, R.AI)]
    with engine.open(seg) as g:
        for (label, rf), (_, tf) in zip(raws, twins):
            got = g.execute(Q.QuerySpec(aggs, filter=rf))
            want = oracle.execute(twin, Q.QuerySpec(aggs, filter=tf))
            assert got.filter_entries_exact == 1 and want.filter_entries_exact, label
            H.assert_results_equal(got, want, check_stats=True)
        # the same Pred object behind two leaves
        p, tp = R.raw_pred(0, lists[0]), R.twin_pred(twin, 0, lists[0])
        f_range = Q.leaf(Q.Pred.dict_range(R.F, 0, 150))
        got = g.execute(Q.QuerySpec(aggs, filter=Q.or_(Q.and_(Q.leaf(p), f_range), Q.not_(Q.leaf(p)))))
        want = oracle.execute(twin, Q.QuerySpec(aggs, filter=Q.or_(Q.and_(Q.leaf(tp), f_range), Q.not_(Q.leaf(tp)))))
        assert got.filter_entries_exact == 1 and want.filter_entries_exact
        H.assert_results_equal(got, want, check_stats=True)
    # set AND range: the leap-frog count of two scan leaves, from the masks themselves
    m0 = R.member_mask(vals, 0, lists[0])
    m1 = (vals["f"] >= 20) & (vals["f"] < 180)
    with engine.open(seg) as g:
        got = g.execute(Q.QuerySpec([(Q.COUNT, -1)], filter=raws[0][1]))
    assert got.stats[1] == H.and_leapfrog_entries([m0, m1]) and got.filter_entries_exact == 1


def test_filter_bitmap_bit_for_bit(engine):
    n = 70_001
    seg, _, vals = R.segments(n, seed=4)
    _, pools = R.column_values(n, seed=4)
    rng = np.random.default_rng(4)
    with engine.open(seg) as g:
        before = g.device_bytes()
        for column in range(4):
            for values in R.value_lists(pools, column, rng)[1:]:
                for exclusive in (False, True):
                    mask = R.member_mask(vals, column, values) != exclusive
                    words, card = g.filter_bitmap(Q.QuerySpec([(Q.COUNT, -1)], filter=Q.leaf(R.raw_pred(column, values, exclusive))))
                    assert card == int(mask.sum())
                    assert np.array_equal(np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool), mask)
        # the leaf's bitmap is scratch the context keeps: pg_segment_device_bytes reports it, once
        grown = g.device_bytes() - before
        assert n // 8 <= grown <= 16 * (n // 8 + 2048)


def test_group_by_and_null_handling(engine):
    n = 60_013
    rng = np.random.default_rng(6)
    null_mask = rng.random(n) < 0.07
    seg, twin, _ = R.segments(n, seed=8, null_mask=null_mask, distinct=200)
    _, pools = R.column_values(n, seed=8, distinct=200)
    values = pools["ri"][rng.choice(len(pools["ri"]), 60, replace=False)].tolist()
    lvalues = pools["rl"][rng.choice(len(pools["rl"]), 60, replace=False)].tolist()
    with engine.open(seg) as g:
        for group_by in ([R.GK], [R.RK], [R.GK, R.RK]):
            for column, vs in ((0, values), (1, lvalues)):
                for exclusive in (False, True):
                    aggs = [(Q.COUNT, -1), (Q.SUM, R.DV), (Q.MAX, R.AI)]
                    got = g.execute(Q.QuerySpec(aggs, filter=Q.leaf(R.raw_pred(column, vs, exclusive)), group_by=group_by))
                    want = oracle.execute(twin, Q.QuerySpec(aggs, filter=Q.leaf(R.twin_pred(twin, column, vs, exclusive)), group_by=group_by))
                    H.assert_results_equal(got, want, check_stats=True)
        # enableNullHandling: IN and NOT IN both leave the null docs of the filtered column out
        for exclusive in (False, True):
            aggs = [(Q.COUNT, -1), (Q.SUM, R.AI)]
            got = g.execute(Q.QuerySpec(aggs, filter=Q.leaf(R.raw_pred(0, values, exclusive)), null_handling=True))
            want = oracle.execute(twin, Q.QuerySpec(aggs, filter=Q.leaf(R.twin_pred(twin, 0, values, exclusive)), null_handling=True))
            H.assert_results_equal(got, want, check_stats=True)


def in_list_of(case):
    """The case's bounds when inclusive plus every multiple of 50 inside the range, formatted as the case formats its literals."""
    lo, hi, inclusive = case["min"], case["max"], case["inclusive"]
    members = sorted({v for v in range(lo - lo % 50, hi + 1, 50) if lo < v < hi} | ({lo, hi} if inclusive else set()))
    floating = case["column"] in ("rawFloatCol", "rawDoubleCol")
    return members, ", ".join(("%d.0" % v) if floating else str(v) for v in members)


def test_sql_in_lists_reproduce_the_range_goldens():
    import torch  # noqa: F401
    host.init_plan_maker(device=0, time_kernels=True)
    data = range_segment()
    segs = [host.HostSegment(data) for _ in range(4)]
    declined = 0
    try:
        cases = [c for c in RANGE_KATS["count_cases"] if c["column"] != "dictionarizedIntCol"]
        assert len(cases) == 32
        for case in cases:
            members, text = in_list_of(case)
            assert 1 <= len(members) <= 11
            for neg, want in (("", case["count"]), (" not", 1000 - case["count"])):
                sql = "select count(*) from testTable where %s%s in (%s)" % (case["column"], neg, text)
                if 0 in members and case["column"] in ("rawFloatCol", "rawDoubleCol"):
                    with pytest.raises(host.HostError) as e:
                        host.execute_sql(segs[:1], sql)
                    assert e.value.status == 2
                    declined += 1
                    continue
                assert int(host.execute_sql(segs[:1], sql)["segments"][0]["intermediate"][0]) == want, sql
                assert int(host.execute_sql(segs, sql, max_execution_threads=4)["combined"]["final"][0]) == 4 * want, sql
        assert declined == 2 * 4
    finally:
        [s.destroy() for s in segs]


def test_batch_of_64_mixed_items(engine):
    n = 30_011
    seg, twin, _ = R.segments(n, seed=13, distinct=400)
    _, pools = R.column_values(n, seed=13, distinct=400)
    rng = np.random.default_rng(13)
    specs = []
    for i in range(64):
        kind = i % 4
        if kind == 0:
            column = (i // 4) % 4
            values = pools[R.FILTER_COLUMNS[column]][rng.choice(400, 50, replace=False)].tolist()      # equal lengths, different values
            specs.append(Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, R.AI)], filter=Q.leaf(R.raw_pred(column, values, bool(i & 16)))))
        elif kind == 1:
            specs.append(Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, R.DV)], filter=Q.leaf(Q.Pred.dict_range(R.F, i, 200))))
        elif kind == 2:
            specs.append(Q.QuerySpec([(Q.SUM, R.DV)], filter=Q.leaf(Q.Pred.dict_set(R.GK, [i % 23, 3], 23))))
        else:
            values = pools["ri"][rng.choice(400, 50, replace=False)].tolist()
            specs.append(Q.QuerySpec([(Q.SUM, R.DV), (Q.COUNT, -1)], filter=Q.and_(Q.leaf(R.raw_pred(0, values)), Q.leaf(Q.Pred.dict_range(R.F, 0, 250)))))
    with engine.open(seg) as g:
        single = [g.execute(s) for s in specs]
        for _ in range(2):                                   # the second call meets the plan cache
            batch = engine.execute_batch([g] * len(specs), specs)
            for (status, got), want in zip(batch, single):
                assert status == _abi.PG_OK
                H.assert_results_equal(got, want, check_stats=True)
                assert got.stats == want.stats


def test_jni_harness_carries_the_value_words(engine):
    from pinot_amd import jni_harness as J
    from test_gpu_jni_harness import same, through_the_c_abi
    n = 20_003
    seg, _, _ = R.segments(n, seed=17, distinct=300)
    _, pools = R.column_values(n, seed=17, distinct=300)
    jvm = J.FakeJvm()
    jvm.call("init", None, C.c_int32(0), C.c_int32(0))
    try:
        with engine.open(seg) as g:
            handle = g.handle if isinstance(g.handle, int) else g.handle.value
            for column in range(4):
                values = pools[R.FILTER_COLUMNS[column]][:77].tolist()
                for exclusive in (False, True):
                    spec = Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, R.AI), (Q.MAX, R.DV)], filter=Q.and_(Q.leaf(R.raw_pred(column, values, exclusive)), Q.leaf(Q.Pred.dict_range(R.F, 0, 250))))
                    assert jvm.query_check(handle, spec) == _abi.PG_OK
                    same(jvm.execute(handle, spec), through_the_c_abi(g, spec))
    finally:
        engine.reinit()


def test_declines(engine):
    n = 5_003
    seg, _, _ = R.segments(n, seed=19)
    with engine.open(seg) as g:
        def statuses(spec):
            res = _abi.pg_result()
            checked = g.check(spec)
            executed = int(g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res)))
            message = (g.lib.pg_last_error() or b"").decode()
            g.lib.pg_result_free(C.byref(res))
            return checked, executed, message

        count = [(Q.COUNT, -1)]
        for pred in (Q.Pred.raw_set(0, range(R.CAP + 1)), Q.Pred.raw_set(1, range(R.CAP + 1)), Q.Pred.raw_set_f64(2, [1.5, -0.0]), Q.Pred.raw_set_f64(3, [0.0]),
                     Q.Pred.raw_set_f64(3, [float("nan"), 2.0]), Q.Pred.raw_set_f64(2, [float("nan")], exclusive=True)):
            checked, executed, message = statuses(Q.QuerySpec(count, filter=Q.leaf(pred)))
            assert (checked, executed) == (_abi.PG_ERR_UNSUPPORTED, _abi.PG_ERR_UNSUPPORTED) and message
        # exactly the cap is served; values an INT column cannot hold are dropped before the cap applies
        assert g.execute(Q.QuerySpec(count, filter=Q.leaf(Q.Pred.raw_set(0, range(R.CAP))))).filter_entries_exact
        assert g.execute(Q.QuerySpec(count, filter=Q.leaf(Q.Pred.raw_set(0, [2 ** 40 + i for i in range(R.CAP + 5)])))).aggregations[0].count == 0
        assert g.execute(Q.QuerySpec(count, filter=Q.leaf(Q.Pred.raw_set(0, [], exclusive=True)))).aggregations[0].count == n
        odd = Q.Pred.raw_set(0, [1, 2])
        odd.set_words = odd.set_words[:3].copy()
        inverted = Q.Pred.raw_set(0, [1, 2])
        inverted.inverted = True
        for pred in (odd, Q.Pred.raw_set(R.DV, [1, 2]), inverted):
            checked, executed, message = statuses(Q.QuerySpec(count, filter=Q.leaf(pred)))
            assert (checked, executed) == (_abi.PG_ERR_INVALID_ARGUMENT, _abi.PG_ERR_INVALID_ARGUMENT) and message
