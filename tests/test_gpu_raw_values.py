"""PERCENTILE and DISTINCTCOUNT on raw (no-dictionary) INT / LONG / FLOAT / DOUBLE columns on the device (scan_collect_kernel /
group_collect_kernel, pg_result_value_counts), through the C ABI.

Expected values: the exact model of tests/raw_value_cases.py (np.unique(values[matching], return_counts=True) in the order image's order,
`matching` from oracle.filter_bitmap), the reference's own statistics and numbers (InterSegmentAggregationSingleValueQueriesTest.testPercentile
/ testDistinctCount over the committed fixture, which do not depend on the encoding), and every other function of a mixed query against the
unchanged oracle.  Lists are compared pair for pair: there are no tolerances.  Every query runs twice: the slot order on the device differs
from run to run, the answers may not.

Where a golden names a column that cannot be raw here: none does -- column1 and column3 are INT columns and both are stored raw; column1 is also
one of the filter's range leaves, which then is a raw INT range leaf (the lane-private filter evaluates it).

The pass is opt-in: the whole module runs under PINOT_GPU_COLLECT=1 (engine.reinit makes the library read its environment again, the way
tests/test_gpu_distinct.py switches its tier); without the switch the raw column is declined as it always was, which the last test holds."""
import ctypes as C
import re

import numpy as np
import pytest

import distinct_cases as D
import helpers as H
import percentile_cases as P
import raw_value_cases as R
from oracle import oracle
from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S

pytestmark = pytest.mark.gpu

PCT, DC = Q.PERCENTILE, Q.DISTINCTCOUNT
SCAN, GROUP = "scan_collect_kernel", "group_collect_kernel"
GRIDS = [None, "1"]          # PINOT_GPU_TEST_CUS: the default grid, and every grid sized for one compute unit (more tiles than waves)


SWITCH = "PINOT_GPU_COLLECT"


@pytest.fixture(scope="module", autouse=True)
def collect_pass_on(engine):
    engine.reinit(**{SWITCH: "1"})
    yield
    engine.reinit(**{SWITCH: None})


class grid:
    def __init__(self, engine, cus):
        self.engine, self.cus = engine, cus

    def __enter__(self):
        self.engine.reinit(PINOT_GPU_TEST_CUS=self.cus)

    def __exit__(self, *exc):
        self.engine.reinit(PINOT_GPU_TEST_CUS=None)


def run_twice(g, spec):
    got, again = g.execute(spec), g.execute(spec)
    R.same_lists(got, again, spec)
    return got


check_others = R.assert_other_functions_equal


# ---- 1. the reference's goldens through the C ABI: column1 and column3 stored raw ----
@pytest.fixture(scope="module")
def golden():
    seg = H.golden_segment(raw_columns=("column1", "column3"))
    d = H.load_golden_columns()
    ci = seg.column_index
    seg.raw_values = {ci("column1"): np.asarray(d["column1"], dtype=np.int32), ci("column3"): np.asarray(d["column3"], dtype=np.int32)}
    return seg, {}          # the segment, and the models of its query shapes (computed once, shared, never changed)


def golden_spec(seg, function, shape, form="physical"):
    filtered, grouped = P.GOLDEN_SHAPES[shape]
    flt = None
    if filtered:
        flt = {"logical": lambda: H.golden_filter(seg), "inverted": lambda: H.golden_filter(seg, inverted=True),
               "physical": lambda: H.golden_filter_physical(seg)}[form]()
    ci = seg.column_index
    return Q.QuerySpec([(function, ci("column1")), (function, ci("column3"))], filter=flt, group_by=[ci("column9")] if grouped else [])


def golden_model(golden, shape):
    seg, cache = golden
    if shape not in cache:
        cache[shape] = R.model(seg, golden_spec(seg, PCT, shape))          # (the lists are the same for both functions)
    return cache[shape]


def finals_of(lists, p, copies=4):
    """(v1, v2) of a golden row from one segment's lists: `copies` identical segments multiply every count; INT values as doubles."""
    return tuple(P.percentile_of_counts(R.double_of_bits(lists[a][0], False), lists[a][1].astype(np.int64) * copies, p) for a in (0, 1))


@pytest.mark.parametrize("shape,form", [("plain", "physical"), ("group", "physical"), ("filter", "logical"), ("filter", "physical"),
                                        ("filter+group", "logical"), ("filter+group", "physical")])
def test_percentile_goldens_on_raw_columns(engine, golden, shape, form):
    seg, _ = golden
    filtered, grouped = P.GOLDEN_SHAPES[shape]
    spec = golden_spec(seg, PCT, shape, form)
    with engine.open(seg) as g:
        got = run_twice(g, spec)
    row = P.GOLDEN_STATS[shape]
    entries = row[1] if (form == "physical" or not filtered) else oracle.execute(seg, R.without_raw_functions(spec)).stats[1]
    assert got.stats == (row[0], entries, row[2], row[3]) and got.filter_entries_exact, (got.stats, row, entries)
    R.assert_lists_equal(got, spec, golden_model(golden, shape), shape)
    for p in (50, 90, 95, 99):
        if grouped:
            finals = max(finals_of({a: v[a].value_counts for a in (0, 1)}, p) for v in got.groups.values())          # ORDER BY v1 DESC, v2 DESC LIMIT 1
        else:
            finals = finals_of({a: got.aggregations[a].value_counts for a in (0, 1)}, p)
        assert finals == P.GOLDEN_VALUES[(p, shape)], (p, shape, finals)
    if shape == "plain":
        assert got.dominant_kernel == SCAN


@pytest.mark.parametrize("shape", ["plain", "filter", "group", "filter+group"])
def test_distinctcount_goldens_on_raw_columns(engine, golden, shape):
    seg, _ = golden
    filtered, grouped = P.GOLDEN_SHAPES[shape]
    spec = golden_spec(seg, DC, shape)
    with engine.open(seg) as g:
        got = run_twice(g, spec)
    R.assert_lists_equal(got, spec, golden_model(golden, shape), shape)
    row = D.GOLDEN_ROWS[shape]
    # (no dictionary answers a raw column: the unfiltered aggregation is a scan, whose statistics are PERCENTILE's plain golden's)
    stats = row["stats"] if shape != "plain" else P.GOLDEN_STATS["plain"]
    assert got.stats == stats and got.filter_entries_exact, (got.stats, stats)
    # a server merges the four identical segments' sets: the union of four equal sets
    if grouped:
        ci = seg.column_index
        c9 = seg.columns[ci("column9")]
        v = got.groups[int(np.searchsorted(c9.dict_values, D.GOLDEN_GROUP_KEY))]
        assert (v[0].count, v[1].count) == (row["v1"], row["v2"])
        assert max((w[0].count, w[1].count) for w in got.groups.values()) == (row["v1"], row["v2"])          # ORDER BY v1 DESC, v2 DESC LIMIT 1
    else:
        assert (got.aggregations[0].count, got.aggregations[1].count) == (row["v1"], row["v2"])


def test_goldens_through_execute_batch(engine, golden):
    seg, _ = golden
    shapes = ["plain", "filter", "filter+group"]
    with engine.open(seg) as g:
        specs = [golden_spec(seg, PCT, s) for s in shapes]
        for shape, spec, (status, got) in zip(shapes, specs, engine.execute_batch([g] * 3, specs)):
            assert status == _abi.PG_OK
            R.assert_lists_equal(got, spec, golden_model(golden, shape), shape)


# ---- 2. prefix / reservation edges ----
@pytest.fixture(scope="module")
def edge_segments():
    cache = {}

    def get(n, pattern):
        if (n, pattern) not in cache:
            seg = R.edge_segment(S, n, pattern)
            models = {}
            cache[(n, pattern)] = (seg, models)
        return cache[(n, pattern)]
    return get


EDGE_COLUMNS = {1: [1], 2: [3, 0], 4: [0, 1, 2, 3]}


@pytest.mark.parametrize("cus", GRIDS)
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_reservation_edges(engine, edge_segments, pattern, cus):
    with grid(engine, cus):
        for n in R.EDGE_SIZES:
            seg, models = edge_segments(n, pattern)
            with engine.open(seg) as g:
                dsid = g.create_doc_set(doc_ids=np.flatnonzero(seg.mask).astype(np.int32)) if pattern == "doc-set" else None
                flt = R.edge_filter(pattern, dsid)
                if pattern != "doc-set":
                    assert np.array_equal(R.matching_docs(seg, Q.QuerySpec([], filter=flt)), seg.mask)
                for num_cols, cols in EDGE_COLUMNS.items():
                    for function in (PCT, DC):
                        spec = Q.QuerySpec([(function, c) for c in cols] + [(Q.COUNT, -1)], filter=flt)
                        if num_cols not in models:
                            models[num_cols] = R.model(seg, spec, match=seg.mask)
                        got = run_twice(g, spec)
                        where = "%d docs %s %d columns f%d" % (n, pattern, num_cols, function)
                        R.assert_lists_equal(got, spec, models[num_cols], where)
                        assert got.aggregations[-1].count == int(seg.mask.sum()) and got.stats[0] == int(seg.mask.sum()), where
                        assert got.stats[2] == got.stats[0] * num_cols and got.stats[3] == n, where
                        # (the longer of the query's kernels: behind an inverted-index leaf index_and_kernel, which lists the tiles, may be it)
                        assert got.dominant_kernel in ((SCAN, "index_and_kernel") if pattern == "tile-list" else (SCAN,)), where


# ---- 3. all four stored types at their edges ----
def type_columns(n, seed=11):
    rng = np.random.default_rng(seed)
    pick = lambda pool, dtype: np.asarray(pool, dtype=dtype)[rng.integers(0, len(pool), n)]
    i32, i64 = np.iinfo(np.int32), np.iinfo(np.int64)
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)
    fnans = np.array([0x7FC00000, 0xFFC00001, 0x7F800001], dtype=np.uint32).view(np.float32)
    big = 1 << 60          # longs that differ only below 2^-53 of their magnitude: one double, distinct values
    return {
        "int-extremes": pick([i32.min, i32.min + 1, -1, 0, 1, i32.max - 1, i32.max], np.int32),
        "long-extremes": pick([i64.min, i64.min + 1, -1, 0, 1, i64.max - 1, i64.max, big, big + 1, big + 2, -big, -big - 1], np.int64),
        "float-edges": np.concatenate([pick([-0.0, 0.0, -np.inf, np.inf, 1.5, -1.5, np.finfo(np.float32).tiny, np.finfo(np.float32).max], np.float32)[: n - 3 * 8], np.tile(fnans, 8)]),
        "double-edges": np.concatenate([pick([-0.0, 0.0, -np.inf, np.inf, 0.1, -0.1, 5e-324, -5e-324, np.finfo(np.float64).max], np.float64)[: n - 4 * 8], np.tile(nans, 8)]),
        "one-value": np.full(n, 7, dtype=np.int64),
        "all-distinct-long": (rng.permutation(n).astype(np.int64) - n // 2) * 1000003,
        "all-distinct-double": rng.permutation(n).astype(np.float64) * 0.5 - n / 4,
        "all-distinct-int": (rng.permutation(n).astype(np.int32) - n // 2),
    }


@pytest.fixture(scope="module")
def type_segment():
    n = 2 * 2048 + 77
    values = type_columns(n)
    names = sorted(values)
    rng = np.random.default_rng(5)
    cols = [S.Column.raw(k, values[k]) if values[k].dtype == np.int32 else S.Column.raw_typed(k, values[k]) for k in names]
    cols.append(S.Column.from_dict_ids("f", np.arange(10, dtype=np.int32), rng.integers(0, 10, n).astype(np.int32)))
    seg = S.SegmentData("raw_types", n, cols)
    seg.raw_values = {i: values[k] for i, k in enumerate(names)}
    seg.names = names
    return seg


@pytest.mark.parametrize("cus", GRIDS)
def test_the_four_stored_types_at_their_edges(engine, type_segment, cus):
    seg = type_segment
    f = len(seg.names)
    with grid(engine, cus), engine.open(seg) as g:
        for flt in (None, Q.leaf(Q.Pred.dict_range(f, 0, 6))):
            for c, name in enumerate(seg.names):
                for function in (PCT, DC):
                    spec = Q.QuerySpec([(function, c)], filter=flt)
                    got = run_twice(g, spec)
                    R.assert_lists_equal(got, spec, R.model(seg, spec), "%s f%d" % (name, function))
        # what the edges are there for
        bits, counts = g.execute(Q.QuerySpec([(DC, seg.names.index("double-edges"))])).aggregations[0].value_counts
        doubles = bits.view(np.float64)
        assert np.isnan(doubles[-1]) and not np.isnan(doubles[:-1]).any() and bits[-1] == 0x7FF8000000000000 and counts[-1] == 32      # one NaN, above +inf
        assert doubles[0] == -np.inf and doubles[-2] == np.inf
        zeros = np.flatnonzero(doubles == 0.0)
        assert len(zeros) == 2 and np.signbit(doubles[zeros[0]]) and not np.signbit(doubles[zeros[1]])                                   # -0.0 below 0.0
        bits, _ = g.execute(Q.QuerySpec([(DC, seg.names.index("long-extremes"))])).aggregations[0].value_counts
        assert len(bits) == 12 and bits[0] == np.iinfo(np.int64).min and bits[-1] == np.iinfo(np.int64).max and (1 << 60) + 1 in bits      # longs on one double stay apart
        v = g.execute(Q.QuerySpec([(PCT, seg.names.index("one-value"))])).aggregations[0]
        assert v.count == seg.num_docs and v.value_counts[0].tolist() == [7] and v.value_counts[1].tolist() == [seg.num_docs]
        v = g.execute(Q.QuerySpec([(DC, seg.names.index("all-distinct-long"))])).aggregations[0]
        assert v.count == seg.num_docs and (v.value_counts[1] == 1).all()


# ---- 4. GROUP BY ----
@pytest.fixture(scope="module")
def group_segment():
    n = 3 * 2048 + 501
    rng = np.random.default_rng(23)
    ids = lambda card: rng.integers(0, card, n).astype(np.int32)
    vi = rng.integers(-300, 300, n).astype(np.int32)
    vl = rng.integers(-50, 50, n).astype(np.int64) * ((1 << 40) + 1)
    vd = rng.integers(-20, 20, n).astype(np.float64) * 0.125
    vf = rng.integers(-9, 9, n).astype(np.float32) * np.float32(1.5)
    key_raw = rng.integers(-40, 60, n).astype(np.int32)
    k3 = ids(3)
    k3[k3 == 1] = 0          # a group without a doc, let alone a match
    k7 = ids(7)
    k7[n - 1] = 6
    k5 = ids(5)
    k5[n - 1] = 4
    k2 = ids(2)
    k2[n - 1] = 1
    k3[n - 1] = 2            # the last doc carries every key's largest dictId: group id = group_id_upper_bound - 1
    cols = [S.Column.raw("ri", vi), S.Column.raw_typed("rl", vl), S.Column.raw_typed("rd", vd), S.Column.raw_typed("rf", vf),        # 0-3
            S.Column.from_dict_ids("k3", np.arange(3, dtype=np.int32), k3), S.Column.from_dict_ids("k7", np.arange(7, dtype=np.int32) * 3, k7),      # 4, 5
            S.Column.from_dict_ids("k5", np.arange(5, dtype=np.int32), k5), S.Column.from_dict_ids("k2", np.arange(2, dtype=np.int32), k2),          # 6, 7
            S.Column.from_dict_ids("f", np.arange(100, dtype=np.int32), ids(100)),                                                                 # 8
            S.Column.raw("kr", key_raw),                                                                                                             # 9: raw INT key
            S.Column.from_dict_ids("v", np.arange(1000, dtype=np.int32), ids(1000))]                                                                # 10
    seg = S.SegmentData("raw_groups", n, cols)
    seg.raw_values = {0: vi, 1: vl, 2: vd, 3: vf}
    seg.key_raw = key_raw
    return seg


@pytest.mark.parametrize("cus", GRIDS)
@pytest.mark.parametrize("function", [PCT, DC])
def test_group_by_dictionary_keys_a_raw_key_and_groups_without_a_match(engine, group_segment, function, cus):
    seg = group_segment
    f_lt = lambda t: Q.leaf(Q.Pred.dict_range(8, 0, t))
    last = Q.leaf(Q.Pred.doc_range(seg.num_docs - 1, seg.num_docs - 1))
    with grid(engine, cus), engine.open(seg) as g:
        cases = [Q.QuerySpec([(function, 0)], filter=f_lt(60), group_by=[5]),                                                       # one key
                 Q.QuerySpec([(function, 1), (Q.SUM, 10), (function, 2), (function, 1)], filter=f_lt(30), group_by=[4, 5, 6, 7]),      # four keys, a column twice, another function
                 Q.QuerySpec([(function, 0), (function, 1), (function, 2), (function, 3)], group_by=[4, 6]),                          # four columns, no filter
                 Q.QuerySpec([(function, 3), (Q.COUNT, -1)], filter=Q.or_(f_lt(2), last), group_by=[4, 5, 6, 7])]                      # few matches: most groups without one
        for spec in cases:
            got = run_twice(g, spec)
            R.assert_lists_equal(got, spec, R.model(seg, spec), "keys %r" % (spec.group_by,))
            check_others(got, seg, spec)
        assert got.group_id_upper_bound == 3 * 7 * 5 * 2 and (3 * 7 * 5 * 2 - 1) in got.groups          # a group id at the upper bound - 1
        # one raw INT key, keyed by offset
        base, is_offset, _ = g.group_key_info(9)
        assert is_offset == 1
        kv = {9: (seg.key_raw, base, int(seg.key_raw.max()) - int(seg.key_raw.min()) + 1)}
        spec = Q.QuerySpec([(function, 2), (Q.COUNT, -1)], filter=f_lt(50), group_by=[9])
        got = run_twice(g, spec)
        R.assert_lists_equal(got, spec, R.model(seg, spec, key_values=kv), "raw key")


def test_mixes_with_other_functions_without_group_by(engine, group_segment):
    seg = group_segment
    flt = Q.leaf(Q.Pred.dict_range(8, 0, 40))
    with engine.open(seg) as g:
        for function in (PCT, DC):
            for spec in (Q.QuerySpec([(Q.COUNT, -1), (function, 1), (Q.SUM, 10), (function, 1), (Q.MAX, 0)], filter=flt),
                         Q.QuerySpec([(function, 2), (Q.AVG, 10), (Q.MIN, 1)]),
                         Q.QuerySpec([(function, 0)], filter=Q.leaf(Q.Pred.raw_range(0, -100, 100)))):          # a raw INT range leaf on the collected column
                got = run_twice(g, spec)
                R.assert_lists_equal(got, spec, R.model(seg, spec))
                check_others(got, seg, spec)


@pytest.mark.parametrize("function", [PCT, DC])
def test_one_raw_int_column_behind_one_in_list_is_still_collected(engine, group_segment, function):
    """ONE raw INT value column behind a filter that is ONE raw IN list is the shape scan_raw_set_kernel takes for SUM / MIN / MAX: the value pass
    must not be lowered for that kernel (it collects nothing: the query failed with "the DISTINCTCOUNT pass returned no sets").  The smallest
    case of what tests/test_gpu_fuzz_values.py found: alone, beside COUNT(*), under GROUP BY, the IN list on the collected column and on another."""
    seg = group_segment
    members = [int(x) for x in np.unique(seg.raw_values[0])[::7]] + [100000]          # present values and an absent one
    keys = [int(x) for x in np.unique(seg.key_raw)[::3]]
    with engine.open(seg) as g:
        for flt in (Q.leaf(Q.Pred.raw_set(0, members)), Q.leaf(Q.Pred.raw_set(9, keys)), Q.leaf(Q.Pred.raw_set(0, members, exclusive=True))):
            for spec in (Q.QuerySpec([(function, 0)], filter=flt), Q.QuerySpec([(function, 0), (Q.COUNT, -1)], filter=flt),
                         Q.QuerySpec([(function, 0)], filter=flt, group_by=[5]), Q.QuerySpec([(function, 0), (Q.MAX, 0)], filter=flt)):
                got = run_twice(g, spec)
                R.assert_lists_equal(got, spec, R.model(seg, spec))
                check_others(got, seg, spec)
                if not spec.group_by and len(spec.aggregations) == 1:
                    assert got.aggregations[0].count > 0


# ---- 5. declines: pg_query_check and pg_execute agree ----
def declined(g, spec, pattern, status_want=_abi.PG_ERR_UNSUPPORTED):
    for call in (lambda: g.lib.pg_query_check(g.handle, C.byref(spec.c)), None):
        if call is not None:
            status = call()
        else:
            res = _abi.pg_result()
            status = g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res))
            g.lib.pg_result_free(C.byref(res))
        message = (g.lib.pg_last_error() or b"").decode()
        assert status == status_want, (status, message)
        assert re.search(pattern, message), message


@pytest.mark.parametrize("function,name", [(PCT, "PERCENTILE"), (DC, "DISTINCTCOUNT")])
def test_declines_name_their_reason(engine, group_segment, function, name):
    seg = group_segment
    other = DC if function == PCT else PCT
    with engine.open(seg) as g:
        declined(g, Q.QuerySpec([(function, 0), (function, 10)]), name + r" on raw column ri and dictionary column v in one query")
        declined(g, Q.QuerySpec([(function, 0), (other, 1)]), r"PERCENTILE beside DISTINCTCOUNT")
        declined(g, Q.QuerySpec([(function, 0)], filter=Q.leaf(Q.Pred.raw_range(1, 0, 1 << 50))), name + r" beside a range predicate on raw LONG / FLOAT / DOUBLE column rl")
        declined(g, Q.QuerySpec([(function, 0)], group_by=[4, 5, 6, 7, 4]), r"more than 4 group-by columns")
        declined(g, Q.QuerySpec([(function, 0)], group_by=[5, 6], num_groups_limit=34), r"above numGroupsLimit 34")
        declined(g, Q.QuerySpec([(function, 0)], group_by=[2]), name + r" grouped by raw column rd, which is not keyed by offset")
        g.execute(Q.QuerySpec([(function, 0)], group_by=[5, 6], num_groups_limit=35))


def test_the_list_bound_is_priced_with_the_docs(engine):
    # 16 bytes x columns x docs (+ 8 x docs under GROUP BY) against PINOT_GPU_GROUP_TABLE_BYTES, by arithmetic: nothing is allocated
    n = 5000
    rng = np.random.default_rng(2)
    seg = S.SegmentData("raw_bound", n, [S.Column.raw("a", rng.integers(0, 9, n).astype(np.int32)), S.Column.raw_typed("b", rng.integers(0, 9, n).astype(np.int64)),
                                         S.Column.from_dict_ids("k", np.arange(4, dtype=np.int32), rng.integers(0, 4, n).astype(np.int32))])
    engine.reinit(PINOT_GPU_GROUP_TABLE_BYTES=str(n * 32 + n * 8 - 1))
    try:
        with engine.open(seg) as g:
            before = g.device_bytes()
            for function, name in ((PCT, "PERCENTILE"), (DC, "DISTINCTCOUNT")):
                declined(g, Q.QuerySpec([(function, 0), (function, 1)], group_by=[2]), name + r" value lists of %d bytes over raw columns exceed the \d+-byte budget" % (n * 40))
            assert g.device_bytes() == before
            g.execute(Q.QuerySpec([(PCT, 0), (PCT, 1)]))          # 32 bytes per doc: fits
            assert g.device_bytes() > before                       # the scratch belongs to the segment's contexts and is counted
    finally:
        engine.reinit(PINOT_GPU_GROUP_TABLE_BYTES=None)
    assert _abi.PG_COLLECT_MAX_BYTES == 1 << 30


def test_a_nullable_raw_column_is_declined_under_null_handling_only(engine):
    n = 4099
    rng = np.random.default_rng(17)
    vals = rng.integers(0, 300, n).astype(np.int32)
    nulls = rng.random(n) < 0.1
    seg = S.SegmentData("raw_nulls", n, [S.Column.raw("vn", vals).with_nulls(nulls), S.Column.raw("v", vals),
                                         S.Column.from_dict_ids("f", np.arange(100, dtype=np.int32), rng.integers(0, 100, n).astype(np.int32))])
    seg.raw_values = {0: vals, 1: vals}
    flt = Q.leaf(Q.Pred.dict_range(2, 0, 40))
    with engine.open(seg) as g:
        for function, name in ((PCT, "PERCENTILE"), (DC, "DISTINCTCOUNT")):
            declined(g, Q.QuerySpec([(function, 0)], filter=flt, null_handling=True), name + r" on column vn, which carries a null value vector, under null handling")
            for spec in (Q.QuerySpec([(function, 0)], filter=flt), Q.QuerySpec([(function, 1), (Q.COUNT, -1)], filter=flt, null_handling=True)):
                R.assert_lists_equal(run_twice(g, spec), spec, R.model(seg, spec))


def test_reserved_flags_are_refused(engine, group_segment):
    with engine.open(group_segment) as g:
        for bit in (26, 27, 28):
            spec = Q.QuerySpec([(PCT, 0)])
            spec.c.flags |= 1 << bit
            declined(g, spec, r"reserved bits", _abi.PG_ERR_INVALID_ARGUMENT)


# ---- 6. the accessors keep to their own encodings; the dictionary forms are what they were ----
def test_each_accessor_answers_its_own_encoding_only(engine, group_segment):
    seg = group_segment
    with engine.open(seg) as g:
        for function, column, raw in ((PCT, 0, True), (DC, 1, True), (PCT, 10, False), (DC, 10, False)):
            spec = Q.QuerySpec([(function, column), (Q.COUNT, -1)], filter=Q.leaf(Q.Pred.dict_range(8, 0, 50)))
            res = _abi.pg_result()
            _abi.check(g.lib, g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res)))
            try:
                bits, counts, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_uint32)(), C.c_int32()
                ids, words = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint32)()
                values = g.lib.pg_result_value_counts(C.byref(res), 0, -1, C.byref(bits), C.byref(counts), C.byref(n))
                pct = g.lib.pg_result_percentile_counts(C.byref(res), 0, -1, C.byref(ids), C.byref(counts), C.byref(n))
                dc = g.lib.pg_result_distinct_dict_ids(C.byref(res), 0, -1, C.byref(words), C.byref(n))
                bad = _abi.PG_ERR_INVALID_ARGUMENT
                assert values == (_abi.PG_OK if raw else bad), (function, column)
                assert pct == (_abi.PG_OK if (not raw and function == PCT) else bad) and dc == (_abi.PG_OK if (not raw and function == DC) else bad)
                # the COUNT(*) beside it, a row of a query without GROUP BY, an index out of range
                assert g.lib.pg_result_value_counts(C.byref(res), 1, -1, C.byref(bits), C.byref(counts), C.byref(n)) == bad
                assert g.lib.pg_result_value_counts(C.byref(res), 0, 0, C.byref(bits), C.byref(counts), C.byref(n)) == bad
                assert g.lib.pg_result_value_counts(C.byref(res), 2, -1, C.byref(bits), C.byref(counts), C.byref(n)) == bad
            finally:
                g.lib.pg_result_free(C.byref(res))


def test_the_dictionary_forms_answer_as_before(engine):
    """The unchanged fixture of the dictionary forms: lists and sets equal their own models (tests/percentile_cases.py, tests/distinct_cases.py),
    the kernels are the dictionary forms' kernels."""
    seg = H.golden_segment()
    with engine.open(seg) as g:
        for shape in ("plain", "filter+group"):
            spec = P.golden_spec(seg, *P.GOLDEN_SHAPES[shape], "physical")
            got = g.execute(spec)
            P.assert_counts_equal(got, seg, spec)
            assert all(v.value_counts is None for v in got.aggregations)
            spec = D.golden_spec(seg, *P.GOLDEN_SHAPES[shape], "physical")
            got = g.execute(spec)
            D.assert_sets_equal(got, seg, spec)
        assert g.execute(P.golden_spec(seg, False, False)).dominant_kernel == "scan_counts_kernel"


# ---- 7. the reference's goldens through SQL: the host mirror over four copies of the raw-column segment (its SQL verbatim) ----
SQL_FILTER = (" WHERE column1 > 100000000 AND column3 BETWEEN 20000000 AND 1000000000 AND column5 = 'gFuH'"
              " AND (column6 < 500000000 OR column11 NOT IN ('t', 'P')) AND daysSinceEpoch = 126164076")
SQL_GROUP_BY = " GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1"
SQL_TAILS = {"plain": "", "filter": SQL_FILTER, "group": SQL_GROUP_BY, "filter+group": SQL_FILTER + SQL_GROUP_BY}


@pytest.fixture(scope="module")
def golden_host_segments():
    import torch  # noqa: F401
    from pinot_amd import host
    host.init_plan_maker(device=0, time_kernels=True)
    data = H.golden_segment(raw_columns=("column1", "column3"))
    segs = [host.HostSegment(data, string_dicts=data.string_dicts) for _ in range(4)]
    yield segs
    for s in segs:
        s.destroy()


def four_segments(stats):
    return (4 * stats[0], 4 * stats[1], 4 * stats[2], 4 * stats[3])


@pytest.mark.parametrize("shape", ["plain", "filter", "group", "filter+group"])
@pytest.mark.parametrize("p,select", [(50, "SELECT PERCENTILE50(column1) AS v1, PERCENTILE50(column3) AS v2 FROM testTable"),
                                      (50, "SELECT PERCENTILE(column1, 50) AS v1, PERCENTILE(column3, '50') AS v2 FROM testTable"),
                                      (90, "SELECT PERCENTILE90(column1) AS v1, PERCENTILE90(column3) AS v2 FROM testTable"),
                                      (95, "SELECT PERCENTILE95(column1) AS v1, PERCENTILE95(column3) AS v2 FROM testTable"),
                                      (99, "SELECT PERCENTILE99(column1) AS v1, PERCENTILE99(column3) AS v2 FROM testTable")])
def test_percentile_goldens_through_sql_over_four_segments(golden_host_segments, p, select, shape):
    from pinot_amd import host
    sql = select + SQL_TAILS[shape]
    out = host.execute_sql(golden_host_segments, sql, max_execution_threads=4)
    st = out["combined"]["stats"]
    stats = four_segments(P.GOLDEN_STATS[shape])
    assert (st["numDocsScanned"], st["numEntriesScannedInFilter"], st["numEntriesScannedPostFilter"], st["numTotalDocs"]) == stats, sql
    want = list(P.GOLDEN_VALUES[(p, shape)])
    if "GROUP BY" in sql:
        assert out["resultTable"]["rows"] == [want], sql
    else:
        assert out["combined"]["final"] == want, sql
        assert [sum(v["counts"]) for v in out["combined"]["intermediate"]] == [stats[0], stats[0]]


@pytest.mark.parametrize("shape", ["plain", "filter", "group", "filter+group"])
def test_distinctcount_goldens_through_sql_over_four_segments(golden_host_segments, shape):
    from pinot_amd import host
    sql = "SELECT DISTINCTCOUNT(column1) AS v1, DISTINCTCOUNT(column3) AS v2 FROM testTable" + SQL_TAILS[shape]
    out = host.execute_sql(golden_host_segments, sql, max_execution_threads=4)
    row = D.GOLDEN_ROWS[shape]
    st = out["combined"]["stats"]
    # (a raw column is always scanned: the unfiltered aggregation's statistics are a scan's, not the dictionary fast path's)
    stats = four_segments(row["stats"] if shape != "plain" else P.GOLDEN_STATS["plain"])
    assert (st["numDocsScanned"], st["numEntriesScannedInFilter"], st["numEntriesScannedPostFilter"], st["numTotalDocs"]) == stats, sql
    if "GROUP BY" in sql:
        assert out["resultTable"]["rows"] == [[row["v1"], row["v2"]]], sql
    else:
        assert out["combined"]["final"] == [float(row["v1"]), float(row["v2"])], sql


# ---- 8. the JNI function over the accessor, executed through the JVM stand-in ----
def test_the_native_method_returns_the_value_lists_with_the_result(engine, golden):
    from pinot_amd import jni_harness as J
    seg, _ = golden
    ci = seg.column_index
    jvm = J.FakeJvm()
    jvm.call("init", None, C.c_int32(0), C.c_int32(0))
    try:
        refs_before = jvm.lib.fj_live_refs()
        handle = jvm.segment_open(seg)
        try:
            for function in (PCT, DC):
                for grouped in (False, True):
                    spec = Q.QuerySpec([(Q.COUNT, -1), (function, ci("column1")), (function, ci("column3"))], filter=H.golden_filter_physical(seg),
                                       group_by=[ci("column9")] if grouped else [])
                    assert jvm.query_check(handle, spec) == _abi.PG_OK
                    result, bits, counts = jvm.execute_with_value_lists(handle, spec)
                    plain = jvm.execute(handle, spec)
                    assert all(np.array_equal(a, b) for a, b in zip(result[1:], plain[1:])) and list(result[0][:4]) == list(plain[0][:4])
                    want = R.model(seg, spec)
                    group_ids = [int(x) for x in result[1]] if grouped else [None]
                    rows = len(group_ids)
                    assert len(bits) == len(counts) == 3 * rows and all(x is None for x in bits[:rows]) and all(x is None for x in counts[:rows])
                    for a in (1, 2):
                        for r, gid in enumerate(group_ids):
                            pairs = want[gid][a] if grouped else want[a]
                            assert np.array_equal(np.asarray(bits[a * rows + r]).view(np.int64), pairs[0])
                            assert np.array_equal(np.asarray(counts[a * rows + r]).view(np.uint32), pairs[1])
                            want_count = int(pairs[1].astype(np.int64).sum()) if function == PCT else len(pairs[0])
                            assert result[2][r * 3 + a] == want_count
            # a dictionary column's aggregation has no value list: the rows of nulls stay
            spec = Q.QuerySpec([(PCT, ci("column6"))])
            _, bits, counts = jvm.execute_with_value_lists(handle, spec)
            assert bits == [None] and counts == [None]
        finally:
            jvm.call("segmentClose", None, C.c_int64(handle))
        assert jvm.lib.fj_live_refs() == refs_before
    finally:
        engine.reinit()


# ---- 9. the switch ----
def test_without_the_switch_a_raw_column_is_declined_as_before(engine, group_segment):
    engine.reinit(**{SWITCH: None})
    try:
        with engine.open(group_segment) as g:
            declined(g, Q.QuerySpec([(PCT, 0)]), r"PERCENTILE on raw \(no-dictionary\) column ri: the collect pass is off \(PINOT_GPU_COLLECT=1 turns it on\)")
            declined(g, Q.QuerySpec([(DC, 1), (Q.COUNT, -1)], group_by=[4]), r"DISTINCTCOUNT on raw \(no-dictionary\) column rl: the collect pass is off")
            g.execute(Q.QuerySpec([(PCT, 10)]))          # the dictionary forms do not ask for it
        for value in ("0", "yes"):
            engine.reinit(**{SWITCH: value})
            with engine.open(group_segment) as g:
                declined(g, Q.QuerySpec([(PCT, 0)]), r"the collect pass is off")
    finally:
        engine.reinit(**{SWITCH: "1"})
