"""The edges of PG_AGG_VARIANCE on the device: non-finite values, the four stored types in one query, the last row of the moment matrices, the
group cap, every plan-time decline from pg_query_check and pg_execute alike, the batch, the accessor, and SQL through the host mirror."""
import ctypes as C
import math
import re
from fractions import Fraction

import numpy as np
import pytest

import distinct_cases as D
import hll_cases as HL
import moments_cases as M
from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S

pytestmark = pytest.mark.gpu

U, I = _abi.PG_ERR_UNSUPPORTED, _abi.PG_ERR_INVALID_ARGUMENT


def answered(g, spec, status, pattern):
    for check_only in (True, False):
        if check_only:
            got = g.lib.pg_query_check(g.handle, C.byref(spec.c))
        else:
            res = _abi.pg_result()
            got = g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res))
            g.lib.pg_result_free(C.byref(res))
        message = (g.lib.pg_last_error() or b"").decode()
        assert got == status, (got, message)
        assert re.search(pattern, message), message


def dict_or_raw(name, values, raw):
    if raw:
        return S.Column.raw_typed(name, values)
    dict_values = HL._sorted_like_java(values)
    bits_of = lambda a: a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
    order = np.argsort(bits_of(dict_values), kind="stable")
    ids = order[np.searchsorted(bits_of(dict_values)[order], bits_of(values))].astype(np.int32)
    return HL.typed_dict_column(S, name, dict_values, ids)


# ---- 1. a value that is not finite makes m2 NaN, in its own row only ----
@pytest.mark.parametrize("raw", [True, False], ids=["raw", "dict"])
@pytest.mark.parametrize("special", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_a_non_finite_value_makes_its_row_nan_and_no_other(engine, special, raw):
    n = 2049
    rng = np.random.default_rng(41)
    values = rng.uniform(-50.0, 50.0, n)
    keys = rng.integers(0, 5, n).astype(np.int32)
    at = 1500
    values[at] = special
    seg = S.SegmentData("moments_special", n, [dict_or_raw("v", values, raw), S.Column.from_dict_ids("k", np.arange(5, dtype=np.int32), keys)])
    finite = values.copy()
    finite[at] = 0.0
    M.set_values(seg, 0, finite)
    with engine.open(seg) as g:
        got = g.execute(Q.QuerySpec([(Q.VARIANCE, 0), (Q.COUNT, -1)]))
        count, total, m2 = got.aggregations[0].moments
        assert count == n and math.isnan(m2), (count, total, m2)
        spec = Q.QuerySpec([(Q.VARIANCE, 0), (Q.COUNT, -1)], group_by=[1])
        got = g.execute(spec)
        for gid, row in got.groups.items():
            count, total, m2 = row[0].moments
            if gid == int(keys[at]):
                assert math.isnan(m2) and count == int((keys == gid).sum()), (gid, count, m2)
            else:
                rows = np.flatnonzero(keys == gid)
                M.assert_one_tuple(row[0], M.exact_of(seg, 0).moments(rows), where="group %d" % gid)


# ---- 2. four columns of four stored types in one query, every value source ----
@pytest.mark.parametrize("raw", [True, False], ids=["raw", "dict"])
def test_four_stored_types_in_one_query(engine, raw):
    seg = M.build_segment(S, 2049, raw)
    col = M.VALUE_COLUMNS.index
    flt = Q.leaf(Q.Pred.dict_range(M.C_FILTER, 100, 900))
    for columns in ([col("int_full"), col("long_wide"), col("float_normal"), col("double_pm1e6")], [col("long_wide"), col("long_1p7e12"), col("long_2p62"), col("int_uniform")]):
        for group_by in ([], [M.C_K2]):
            spec = Q.QuerySpec([(Q.VARIANCE, c) for c in columns] + [(Q.SUM, c) for c in columns] + [(Q.COUNT, -1)], filter=flt, group_by=group_by)
            with engine.open(seg) as g:
                got = g.execute(spec)
            M.assert_moments(got, seg, spec, where="%s %s %s" % ("raw" if raw else "dict", columns, group_by))
            # the same column twice shares one slot of the pass
            twice = Q.QuerySpec([(Q.VARIANCE, columns[0]), (Q.VARIANCE, columns[1]), (Q.VARIANCE, columns[0])], filter=flt, group_by=group_by)
            with engine.open(seg) as g:
                got = g.execute(twice)
            M.assert_moments(got, seg, twice)
            rows = got.groups.values() if group_by else [got.aggregations]
            assert all(np.float64(r[0].moments[2]).tobytes() == np.float64(r[2].moments[2]).tobytes() for r in rows)


# ---- 3. the last row of the matrices, a last group of one doc ----
@pytest.mark.parametrize("raw", [True, False], ids=["raw", "dict"])
def test_the_last_row_of_the_matrix_and_a_group_of_one_doc(engine, raw):
    n = 2049
    rng = np.random.default_rng(43)
    values = rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int64) * 1001
    k1 = rng.integers(0, 6, n).astype(np.int32)
    k2 = rng.integers(0, 10, n).astype(np.int32)
    k1[-1], k2[-1] = 6, 10                                                # the largest dictId of either key: once, on the last doc
    seg = S.SegmentData("moments_last_row", n, [dict_or_raw("v", values, raw), S.Column.from_dict_ids("k1", np.arange(7, dtype=np.int32), k1),
                                                S.Column.from_dict_ids("k2", np.arange(11, dtype=np.int32) * 2, k2)])
    M.set_values(seg, 0, values)
    spec = Q.QuerySpec([(Q.VARIANCE, 0), (Q.SUM, 0), (Q.COUNT, -1)], group_by=[1, 2])
    with engine.open(seg) as g:
        got = g.execute(spec)
    M.assert_moments(got, seg, spec)
    last = 7 * 11 - 1
    assert got.group_id_upper_bound == 77 and max(got.groups) == last
    assert got.groups[last][0].moments == (1, float(values[-1]), 0.0)


# ---- 4. the group cap, on both sides, from pg_query_check alone ----
def test_the_group_cap_on_both_sides(engine):
    """PG_MOMENTS_GROUP_MAX_BYTES: raw group ids x 24 bytes x distinct VARIANCE columns.  3640 x 4097 ids x 72 bytes are 64 bytes below 2^30:
    accepted; 171 x 87211 ids (one more) are 8 bytes above: declined.  Nothing is allocated or executed."""
    n = 2049
    rng = np.random.default_rng(47)
    key = lambda name, card: S.Column.from_dict_ids(name, np.arange(card, dtype=np.int32), rng.integers(0, card, n).astype(np.int32))
    value = lambda name: S.Column.raw_typed(name, rng.integers(-1000, 1000, n).astype(np.int32))
    seg = S.SegmentData("moments_cap", n, [value("a"), value("b"), key("dv", 50), key("k3640", 3640), key("k4097", 4097), key("k171", 171), key("k87211", 87211)])
    assert 3640 * 4097 + 1 == 171 * 87211 and 3640 * 4097 * 72 <= _abi.PG_MOMENTS_GROUP_MAX_BYTES < 171 * 87211 * 72
    aggs = [(Q.VARIANCE, 0), (Q.VARIANCE, 1), (Q.VARIANCE, 2), (Q.VARIANCE, 0)]
    with engine.open(seg) as g:
        before = g.device_bytes()
        spec = Q.QuerySpec(aggs, group_by=[3, 4], num_groups_limit=20000000)
        status = g.lib.pg_query_check(g.handle, C.byref(spec.c))
        assert status == _abi.PG_OK, (status, (g.lib.pg_last_error() or b"").decode())
        spec = Q.QuerySpec(aggs, group_by=[5, 6], num_groups_limit=20000000)
        status = g.lib.pg_query_check(g.handle, C.byref(spec.c))
        message = (g.lib.pg_last_error() or b"").decode()
        assert status == U, (status, message)
        assert "VARIANCE moment matrices of %d bytes exceed PG_MOMENTS_GROUP_MAX_BYTES (%d)" % (171 * 87211 * 72, 1 << 30) in message, message
        assert g.device_bytes() == before
        # the budget of the group tables bounds it too
        engine.reinit(PINOT_GPU_GROUP_TABLE_BYTES=str(50 * 24 * 2 - 1))
        try:
            answered(g, Q.QuerySpec([(Q.VARIANCE, 0), (Q.VARIANCE, 1)], group_by=[2]), U, r"VARIANCE moment matrices of 2400 bytes exceed the 2399-byte budget \(PINOT_GPU_GROUP_TABLE_BYTES\)")
        finally:
            engine.reinit(PINOT_GPU_GROUP_TABLE_BYTES=None)


# ---- 5. declines: the same status and message from pg_query_check and pg_execute ----
def test_declines_name_their_reason(engine):
    n = 2049
    rng = np.random.default_rng(53)
    raw_int = lambda name: S.Column.raw_typed(name, rng.integers(-1000, 1000, n).astype(np.int32))
    key = lambda name, card: S.Column.from_dict_ids(name, np.arange(card, dtype=np.int32), rng.integers(0, card, n).astype(np.int32))
    nullable = S.Column.raw_typed("rn", rng.integers(0, 50, n).astype(np.int32)).with_nulls(rng.random(n) < 0.2)
    nullable_key = key("kn", 6).with_nulls(rng.random(n) < 0.2)
    cols = [raw_int("r0"), raw_int("r1"), raw_int("r2"), raw_int("r3"), raw_int("r4"),                                 # 0-4
            key("d", 100),                                                                                             # 5
            S.Column.raw_typed("rl", rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64)),                             # 6
            nullable,                                                                                                  # 7
            key("k", 9),                                                                                               # 8
            S.Column.raw_typed("rf", rng.standard_normal(n).astype(np.float32)),                                       # 9
            key("k60000", 60000), key("k50000", 50000),                                                                # 10, 11
            key("ka", 3), key("kb", 3), key("kc", 3), key("kd", 3),                                                    # 12-15
            nullable_key,                                                                                              # 16
            S.Column.raw_typed("rbig", (2 ** 62 + rng.integers(0, 2 ** 62 - 1, n)).astype(np.int64))]                  # 17
    seg = S.SegmentData("moments_declines", n, cols)
    V = Q.VARIANCE
    with engine.open(seg) as g:
        answered(g, Q.QuerySpec([(V, 7)], null_handling=True), U, r"VARIANCE on column rn, which carries a null value vector, under null handling -- CPU plan")
        g.execute(Q.QuerySpec([(V, 7)]))                                # (without the option the null vector is not looked at)
        g.execute(Q.QuerySpec([(V, 0)], null_handling=True))            # (nor is a column without one declined under the option)
        answered(g, Q.QuerySpec([(V, 0), (Q.DISTINCTCOUNT, 5)]), U, r"DISTINCTCOUNT beside VARIANCE in one query -- CPU plan")
        answered(g, Q.QuerySpec([(Q.PERCENTILE, 5), (V, 0)]), U, r"PERCENTILE beside VARIANCE in one query -- CPU plan")
        answered(g, Q.QuerySpec([(V, 5), (Q.hll(12), 0)]), U, r"DISTINCTCOUNTHLL beside VARIANCE in one query -- CPU plan")
        answered(g, Q.QuerySpec([(V, c) for c in range(5)]), U, r"more than 4 VARIANCE columns -- CPU plan")
        g.execute(Q.QuerySpec([(V, c) for c in (0, 1, 2, 3, 0, 1)]))     # (six aggregations over four columns run)
        answered(g, Q.QuerySpec([(V, 0)], filter=Q.leaf(Q.Pred.raw_range(6, -5, 5))), U, r"VARIANCE beside a range predicate on raw LONG / FLOAT / DOUBLE column rl -- CPU plan")
        g.execute(Q.QuerySpec([(V, 6)], filter=Q.leaf(Q.Pred.raw_range(0, -5, 5))))      # (a range on a raw INT column is in the pass's filter)
        # GROUP BY outside the conditions PG_AGG_DISTINCTCOUNT states
        answered(g, Q.QuerySpec([(V, 0)], group_by=[10, 11], num_groups_limit=2 ** 31 - 1), U, r"VARIANCE grouped over a key space of kind \d \(raw keys beyond an int: the hashed holders\) -- CPU plan")
        answered(g, Q.QuerySpec([(V, 0)], group_by=[5, 8], num_groups_limit=899), U, r"VARIANCE grouped over 900 raw keys, above numGroupsLimit 899 \(the limit could bind\) -- CPU plan")
        g.execute(Q.QuerySpec([(V, 0)], group_by=[5, 8], num_groups_limit=900))
        answered(g, Q.QuerySpec([(V, 0)], group_by=[9]), U, r"VARIANCE grouped by raw column rf, which is not keyed by offset -- CPU plan")
        g.execute(Q.QuerySpec([(V, 1)], group_by=[0]))                  # (a raw INT key is keyed by offset)
        answered(g, Q.QuerySpec([(V, 0)], group_by=[12, 13, 14, 15, 8]), U, r"VARIANCE with more than 4 group-by columns -- CPU plan")
        g.execute(Q.QuerySpec([(V, 0)], group_by=[12, 13, 14, 15]))
        answered(g, Q.QuerySpec([(V, 0)], group_by=[16], null_handling=True), U, r"VARIANCE grouped by nullable column kn under null handling -- CPU plan")
        g.execute(Q.QuerySpec([(V, 0)], group_by=[16]))
        # a raw LONG column whose group sums could wrap int64 without a way back
        answered(g, Q.QuerySpec([(V, 17)], group_by=[8]), U, r"VARIANCE grouped on raw LONG column rbig, whose group sums could wrap int64 beyond repair -- CPU plan")
        g.execute(Q.QuerySpec([(V, 17)]))
        # bits above the low byte of the function word: not a query at all
        answered(g, Q.QuerySpec([(V | (8 << 8), 0)]), I, r"sets bits above the function's byte")
        # whatever the ordinary query declines
        answered(g, Q.QuerySpec([(V, 0), (Q.SUM, 1), (Q.SUM, 2), (Q.SUM, 3), (Q.SUM, 4)]), U, r"more than 4 aggregated columns")


# ---- 6. a VARIANCE item of pg_execute_batch runs as a pg_execute of its own ----
def test_a_batch_with_a_variance_item_among_ordinary_ones(engine):
    seg = M.build_segment(S, 2049, raw=True)
    flt = Q.leaf(Q.Pred.dict_range(M.C_FILTER, 0, 600))
    ordinary = Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, 0)], filter=flt)
    variance = Q.QuerySpec([(Q.VARIANCE, 0), (Q.VARIANCE, 2), (Q.COUNT, -1)], filter=flt, group_by=[M.C_K1])      # (INT and LONG: their group sums are exact)
    grouped = Q.QuerySpec([(Q.SUM, 0)], filter=flt, group_by=[M.C_K1])
    with engine.open(seg) as g:
        out = engine.execute_batch([g, g, g], [ordinary, variance, grouped])
        singles = [g.execute(spec) for spec in (ordinary, variance, grouped)]
    assert [status for status, _ in out] == [_abi.PG_OK] * 3
    M.assert_moments(out[1][1], seg, variance)
    for (_, got), want in zip(out, singles):
        assert sorted(got.groups) == sorted(want.groups) and got.stats == want.stats
        rows = [(got.aggregations, want.aggregations)] + [(got.groups[gid], want.groups[gid]) for gid in want.groups]
        for a_row, b_row in rows:
            assert [(v.count, v.sum, v.sum_i64) for v in a_row] == [(v.count, v.sum, v.sum_i64) for v in b_row]
            # (a grouped m2 adds in no fixed order: the single execute and the batch item agree to the tolerance, which assert_moments held both to)
            assert [v.moments is None for v in a_row] == [v.moments is None for v in b_row]


# ---- 7. the accessor ----
def test_the_accessor_rejects_what_is_not_a_tuple(engine):
    seg = M.build_segment(S, 2049, raw=True)
    with engine.open(seg) as g:
        for group_by, good_row, bad_rows in (([], -1, (0, 1, -2)), ([M.C_K2], 0, (-1, 5, 99))):
            spec = Q.QuerySpec([(Q.COUNT, -1), (Q.VARIANCE, 0), (Q.AVG, 0)], group_by=group_by)
            res = _abi.pg_result()
            _abi.check(g.lib, g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res)))
            try:
                n, total, m2 = C.c_int64(), C.c_double(), C.c_double()
                call = lambda a, row: g.lib.pg_result_moments(C.byref(res), a, row, C.byref(n), C.byref(total), C.byref(m2))
                assert call(1, good_row) == _abi.PG_OK and n.value > 0 and m2.value > 0.0
                for a, row in [(0, good_row), (2, good_row), (3, good_row), (-1, good_row)] + [(1, row) for row in bad_rows]:
                    assert call(a, row) == I, (group_by, a, row)
                assert g.lib.pg_result_moments(C.byref(res), 1, good_row, None, C.byref(total), C.byref(m2)) == I
            finally:
                g.lib.pg_result_free(C.byref(res))


# ---- 8. SQL through the host mirror, two segments ----
@pytest.fixture(scope="module")
def host_segments():
    import torch  # noqa: F401
    from pinot_amd import host
    host.init_plan_maker(device=0, time_kernels=True)
    data = [M.build_segment(S, 2049, raw=False, seed=0), M.build_segment(S, 2047, raw=True, seed=1)]
    segs = [host.HostSegment(d) for d in data]
    yield data, segs
    for s in segs:
        s.destroy()


def union_model(data, column, where=None, keys=()):
    """{key tuple: (n, sum, E, X)} of a column's values over both segments: `where` = largest flt value admitted (exclusive), keys = key column indexes."""
    col = M.VALUE_COLUMNS.index(column)
    doubles = np.concatenate([M.as_doubles(M.values_of(d, col)) for d in data])
    mask = np.ones(doubles.shape[0], dtype=bool)
    if where is not None:
        mask &= np.concatenate([D.dict_ids_of(d, M.C_FILTER) for d in data]) < where
    exact = M.Exact(doubles)
    if not keys:
        return {(): exact.moments(mask)}
    key_values = [np.concatenate([np.asarray(d.columns[k].dict_values)[D.dict_ids_of(d, k)] for d in data]) for k in keys]
    out = {}
    for key in sorted(set(zip(*[kv[mask].tolist() for kv in key_values]))):
        rows = mask.copy()
        for kv, v in zip(key_values, key):
            rows &= kv == v
        out[key] = exact.moments(rows)
    return out


def assert_final(kind, got, want):
    n, _, e, x_max = want
    exact = M.final(kind, (n, 0.0, float(e)))
    if n == 0 or (kind.endswith("samp") and n == 1):
        assert float(got) == exact == float("-inf")
        return
    relative = float(M.tol(n, e, x_max) / e) if e > 0 else 0.0
    if kind.startswith("stddev"):
        relative /= 2.0
    print("%s: n=%d got %r exact %r relative bound %.3e" % (kind, n, got, exact, relative))
    assert abs(got - exact) <= relative * exact, (kind, got, exact, relative)


def test_four_queries_through_sql_over_two_segments(host_segments):
    from pinot_amd import host
    data, segs = host_segments
    out = host.execute_sql(segs, "SELECT VAR_POP(double_pm1e6), STDDEV_SAMP(long_1p7e12), COUNT(*) FROM t")
    assert out["combined"]["columns"] == ["varpop(double_pm1e6)", "stddevsamp(long_1p7e12)", "count(*)"]
    assert_final("varpop", out["combined"]["final"][0], union_model(data, "double_pm1e6")[()])
    assert_final("stddevsamp", out["combined"]["final"][1], union_model(data, "long_1p7e12")[()])
    assert out["combined"]["final"][2] == 2049 + 2047
    st = out["combined"]["stats"]
    assert [st["numDocsScanned"], st["numEntriesScannedPostFilter"], st["numTotalDocs"]] == [4096, 2 * 4096, 4096]

    out = host.execute_sql(segs, "SELECT STD_DEV_POP(float_normal), var_samp(long_1p7e12), var_samp(long_2p62) FROM t WHERE flt < 500")
    assert_final("stddevpop", out["combined"]["final"][0], union_model(data, "float_normal", 500)[()])
    assert_final("varsamp", out["combined"]["final"][1], union_model(data, "long_1p7e12", 500)[()])
    # LONG values near 2^62 are a family on which the reference's own arithmetic leaves the tolerance (tests/test_moments_cpu.py), and the combine IS
    # the reference's apply(VarianceTuple): its delta of two averages near 2^62 carries an absolute error of about 2^62 u n.  So the union's final is
    # not held to the exact model here; every SEGMENT's tuple is, and the combined tuple to the restated merge of those, bit for bit.
    col = M.VALUE_COLUMNS.index("long_2p62")
    tuples = []
    for d, block in zip(data, out["segments"]):
        t = block["intermediate"][2]
        want = M.Exact(M.as_doubles(M.values_of(d, col))).moments(D.dict_ids_of(d, M.C_FILTER) < 500)
        assert t["count"] == want[0] and abs(Fraction(float(t["m2"])) - want[2]) <= M.tol(want[0], want[2], want[3]), (t, want)
        tuples.append((t["count"], float(t["sum"]), float(t["m2"])))
    merged = M.merge_tuples(tuples)
    got = out["combined"]["intermediate"][2]
    assert (got["count"], np.float64(got["sum"]).tobytes(), np.float64(got["m2"]).tobytes()) == (merged[0], np.float64(merged[1]).tobytes(), np.float64(merged[2]).tobytes())
    assert out["combined"]["final"][2] == M.final("varsamp", merged)

    out = host.execute_sql(segs, "SELECT k1, VAR_SAMP(int_uniform), STDDEV_POP(double_unit) FROM t GROUP BY k1 ORDER BY k1 LIMIT 10")
    want_a, want_b = union_model(data, "int_uniform", keys=[M.C_K1]), union_model(data, "double_unit", keys=[M.C_K1])
    assert [row[0] for row in out["resultTable"]["rows"]] == [key[0] for key in sorted(want_a)]
    for row in out["resultTable"]["rows"]:
        assert_final("varsamp", row[1], want_a[(row[0],)])
        assert_final("stddevpop", row[2], want_b[(row[0],)])

    out = host.execute_sql(segs, "SELECT STDDEV_POP(long_wide) AS s, VAR_POP(int_const7) FROM t WHERE flt < 700 GROUP BY k1, k2 ORDER BY s DESC LIMIT 50")
    want_a, want_b = union_model(data, "long_wide", 700, keys=[M.C_K1, M.C_K2]), union_model(data, "int_const7", 700, keys=[M.C_K1, M.C_K2])
    reduced = out["reduced"]
    assert sorted((row[0], row[1]) for row in reduced) == sorted(want_a) and len(reduced) == 35
    assert [row[2] for row in reduced] == sorted((row[2] for row in reduced), reverse=True)
    for row in reduced:
        assert_final("stddevpop", row[2], want_a[(row[0], row[1])])
        assert row[3] == 0.0 and want_b[(row[0], row[1])][2] == 0


def test_datatable_bytes_of_a_tuple_are_declined(host_segments):
    from pinot_amd import host
    _, segs = host_segments
    with pytest.raises(host.HostError) as e:
        host.execute_sql_datatable(segs[:1], "SELECT VAR_POP(double_pm1e6) FROM t")
    assert e.value.status == 2 and "VarianceTuple" in str(e.value)


def test_string_columns_and_filtered_aggregations_keep_the_cpu_plan(host_segments):
    import helpers as H
    from pinot_amd import host
    _, segs = host_segments
    golden = H.golden_segment()
    seg = host.HostSegment(golden, string_dicts=golden.string_dicts)
    try:
        with pytest.raises(host.HostError) as e:
            host.execute_sql([seg], "SELECT STDDEV_SAMP(column5) FROM testTable")
        assert e.value.status == 2 and "stddevsamp(column5) on a STRING column keeps the CPU plan" in str(e.value)
    finally:
        seg.destroy()
    with pytest.raises(host.HostError) as e:
        host.execute_sql(segs, "SELECT VAR_POP(double_pm1e6) FILTER (WHERE flt < 5), COUNT(*) FROM t")
    assert e.value.status == 2 and "varpop(double_pm1e6) in a query with FILTER" in str(e.value)


# ---- 9. the JNI function over the accessor, executed through the JVM stand-in ----
def test_the_native_method_returns_the_tuples_with_the_result(engine):
    from pinot_amd import jni_harness as J
    jvm = J.FakeJvm()
    jvm.call("init", None, C.c_int32(0), C.c_int32(0))
    try:
        refs_before = jvm.lib.fj_live_refs()
        for raw in (True, False):
            seg = M.build_segment(S, 2049, raw)
            handle = jvm.segment_open(seg)
            try:
                for group_by in ([], [M.C_K1]):
                    spec = Q.QuerySpec([(Q.COUNT, -1), (Q.VARIANCE, 0), (Q.VARIANCE, 2), (Q.SUM, 0)], filter=Q.leaf(Q.Pred.dict_range(M.C_FILTER, 0, 600)), group_by=group_by)
                    assert jvm.query_check(handle, spec) == _abi.PG_OK
                    result, m2s = jvm.execute_with_moments(handle, spec)
                    plain = jvm.execute(handle, spec)
                    assert all(np.array_equal(a, b) for a, b in zip(result[1:], plain[1:])) and list(result[0][:4]) == list(plain[0][:4])
                    want = M.model(seg, spec)
                    group_ids = [int(x) for x in result[1]] if group_by else [None]
                    rows = len(group_ids)
                    assert m2s.dtype == np.float64 and len(m2s) == 4 * rows and not np.any(m2s[:rows]) and not np.any(m2s[3 * rows:])
                    for a in (1, 2):
                        for r, gid in enumerate(group_ids):
                            n, total, e, x_max = want[gid][a] if group_by else want[a]
                            # counts and sums of the result arrays: row-major; the integer columns' sums are exact
                            assert int(result[2][r * 4 + a]) == n and float(result[3][r * 4 + a]) == float(total), (raw, group_by, a, gid)
                            assert abs(Fraction(float(m2s[a * rows + r])) - e) <= M.tol(n, e, x_max), (raw, group_by, a, gid)
            finally:
                jvm.call("segmentClose", None, C.c_int64(handle))
        assert jvm.lib.fj_live_refs() == refs_before
    finally:
        engine.reinit()
