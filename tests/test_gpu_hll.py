"""DISTINCTCOUNTHLL on the device (PG_AGG_DISTINCTCOUNTHLL / PG_AGG_HLL(log2m), pg_result_hll_registers), through the C ABI and the host mirror.

Expected values: the reference's own numbers (InterSegmentAggregationSingleValueQueriesTest.testDistinctCountHLL :261-284 over the committed
fixture) and the numpy model of tests/hll_cases.py over the docs oracle.filter_bitmap matches.  What crosses the ABI is integers: registers are
compared byte for byte, estimates exactly; there is no tolerance anywhere."""
import ctypes as C
import re

import numpy as np
import pytest

import distinct_cases as D
import helpers as H
import hll_cases as HL
from oracle import oracle
from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S

pytestmark = pytest.mark.gpu

SCAN_DICT, GROUP_DICT = "scan_distinct_kernel", "group_distinct_kernel"
SCAN_RAW, GROUP_RAW = "scan_hll_kernel", "group_hll_kernel"
RAW_GOLDEN_COLUMNS = ("column1", "column3")


@pytest.fixture(scope="module")
def goldens():
    """The fixture segment in both forms (column1 / column3 dictionary-encoded, or stored raw) and the model of its four queries: computed once,
    shared, never changed.  The values are the same in both forms, so one model serves both."""
    dict_seg = H.golden_segment()
    raw_seg = H.golden_segment(raw_columns=RAW_GOLDEN_COLUMNS)
    columns = H.load_golden_columns()
    for name in RAW_GOLDEN_COLUMNS:
        HL.set_values(raw_seg, raw_seg.column_index(name), columns[name])
    models = {(f, g): HL.model(dict_seg, HL.golden_spec(dict_seg, f, g)) for _, f, g in HL.GOLDEN_CASES}
    return {"dict": dict_seg, "raw": raw_seg, "models": models}


def pass_kernel_or_the_ordinary_one(g, spec, got, pass_kernel):
    """Under GROUP BY a query runs twice -- the ordinary group-by (every HLL as COUNT(*)), then the HLL pass -- and dominant_kernel names whichever
    kernel took longer.  It is one of exactly two names: the pass's kernel, or the kernel the ordinary query reports when it runs alone."""
    ordinary = g.execute(HL.without_hll(spec)).dominant_kernel
    assert ordinary not in (pass_kernel, ""), ordinary
    assert got.dominant_kernel in (pass_kernel, ordinary), (got.dominant_kernel, pass_kernel, ordinary)


def golden_row(filtered, grouped):
    return HL.GOLDEN_ROWS[next(name for name, f, g in HL.GOLDEN_CASES if (f, g) == (filtered, grouped))]


def check_golden_registers(got, goldens, form, filtered, grouped):
    seg = goldens[form]
    row = golden_row(filtered, grouped)
    HL.assert_registers_equal(got, seg, HL.golden_spec(seg, filtered, grouped, "physical"), want=goldens["models"][(filtered, grouped)])
    if grouped:
        top_id = D.golden_group_id(goldens["dict"])
        pairs = {gid: HL.golden_pair({0: v[0].hll_registers, 1: v[1].hll_registers}) for gid, v in got.groups.items()}
        assert pairs[top_id] == (row["v1"], row["v2"])
        assert max(pairs, key=lambda gid: pairs[gid]) == top_id          # ORDER BY v1 DESC, v2 DESC LIMIT 1 picks that group
    else:
        assert HL.golden_pair({0: got.aggregations[0].hll_registers, 1: got.aggregations[1].hll_registers}) == (row["v1"], row["v2"])


# ---- 1. the reference's goldens through the C ABI, dictionary form ----
@pytest.mark.parametrize("name,filtered,grouped", HL.GOLDEN_CASES)
def test_goldens_on_dictionary_columns(engine, goldens, name, filtered, grouped):
    seg = goldens["dict"]
    spec = HL.golden_spec(seg, filtered, grouped, "physical")
    with engine.open(seg) as g:
        got = g.execute(spec)
        if grouped:
            pass_kernel_or_the_ordinary_one(g, spec, got, GROUP_DICT)
    check_golden_registers(got, goldens, "dict", filtered, grouped)
    assert got.stats == HL.GOLDEN_ROWS[name]["stats"] and got.filter_entries_exact, got.stats
    if not filtered and not grouped:
        assert got.dominant_kernel_ms == 0.0                            # the whole dictionaries folded: nothing was scanned
    elif not grouped:
        assert got.dominant_kernel == SCAN_DICT, got.dominant_kernel        # the pass alone: its kernel is the query's


# ---- 2. the same through SQL: the host mirror over four copies of the segment ----
SQL_QUERY = "SELECT DISTINCTCOUNTHLL(column1) AS v1, DISTINCTCOUNTHLL(column3) AS v2 FROM testTable"
SQL_FILTER = (" WHERE column1 > 100000000 AND column3 BETWEEN 20000000 AND 1000000000 AND column5 = 'gFuH'"
              " AND (column6 < 500000000 OR column11 NOT IN ('t', 'P')) AND daysSinceEpoch = 126164076")
SQL_GROUP_BY = " GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1"
SQL_GOLDENS = [(SQL_QUERY, 120000, 0, 0, 120000, [5977, 23825]),
               (SQL_QUERY + SQL_FILTER, 24516, 252256, 49032, 120000, [1886, 4492]),
               (SQL_QUERY + SQL_GROUP_BY, 120000, 0, 360000, 120000, [3592, 11889]),
               (SQL_QUERY + SQL_FILTER + SQL_GROUP_BY, 24516, 252256, 73548, 120000, [1324, 3197])]


@pytest.fixture(scope="module")
def golden_host_segments():
    import torch  # noqa: F401
    from pinot_amd import host
    host.init_plan_maker(device=0, time_kernels=True)
    data = H.golden_segment()
    segs = [host.HostSegment(data, string_dicts=data.string_dicts) for _ in range(4)]
    yield segs
    for s in segs:
        s.destroy()


@pytest.mark.parametrize("case", range(4))
def test_goldens_through_sql_over_four_segments(golden_host_segments, case):
    from pinot_amd import host
    sql, docs, in_filter, post_filter, total, row = SQL_GOLDENS[case]
    out = host.execute_sql(golden_host_segments, sql, max_execution_threads=4)
    st = out["combined"]["stats"]
    assert [st["numDocsScanned"], st["numEntriesScannedInFilter"], st["numEntriesScannedPostFilter"], st["numTotalDocs"]] == [docs, in_filter, post_filter, total], sql
    if "GROUP BY" in sql:
        assert out["resultTable"]["rows"] == [row], sql
        assert all(isinstance(x, int) for x in out["resultTable"]["rows"][0])
    else:
        assert out["combined"]["final"] == row, sql                      # four copies of the segment merge to the segment's registers
        assert [len(v["registers"]) for v in out["combined"]["intermediate"]] == [256, 256]


def test_datatable_bytes_of_a_sketch_are_declined(golden_host_segments):
    from pinot_amd import host
    with pytest.raises(host.HostError) as e:
        host.execute_sql_datatable(golden_host_segments[:1], SQL_QUERY + SQL_FILTER)
    assert e.value.status == 2 and "DISTINCTCOUNTHLL" in str(e.value)


# ---- 3. the goldens on raw columns: scan_hll_kernel / group_hll_kernel ----
@pytest.mark.parametrize("name,filtered,grouped", HL.GOLDEN_CASES)
def test_goldens_on_raw_columns(engine, goldens, name, filtered, grouped):
    seg = goldens["raw"]
    spec = HL.golden_spec(seg, filtered, grouped, "physical")
    with engine.open(seg) as g:
        got = g.execute(spec)
        if grouped:
            pass_kernel_or_the_ordinary_one(g, spec, got, GROUP_RAW)
    check_golden_registers(got, goldens, "raw", filtered, grouped)
    if not grouped:
        assert got.dominant_kernel == SCAN_RAW, got.dominant_kernel          # the pass alone: its kernel is the query's
    # a raw column is always scanned: the statistics are those of raw DISTINCTCOUNT -- docs and total as the reference's, every projected column read
    # per scanned doc, the filter's entries what the oracle counts for this filter over raw columns
    row = HL.GOLDEN_ROWS[name]
    want = oracle.execute(seg, HL.without_hll(spec))
    assert got.stats[0] == row["stats"][0] and got.stats[3] == row["stats"][3]
    assert got.stats[2] == got.stats[0] * D.projected_columns(spec)
    if got.filter_entries_exact and want.filter_entries_exact:
        assert got.stats[1] == want.stats[1]


# ---- 4. edges: sizes around a tile, the four stored types, three register counts, every kind of filter the body evaluates ----
def hll_specs(seg, log2m=8):
    return [(Q.hll(log2m), HL.E_INT), (Q.hll(log2m), HL.E_LONG), (Q.hll(log2m), HL.E_FLOAT), (Q.hll(log2m), HL.E_DOUBLE)]


@pytest.mark.parametrize("raw", [True, False], ids=["raw", "dict"])
@pytest.mark.parametrize("num_docs", HL.EDGE_SIZES)
def test_edges(engine, monkeypatch, num_docs, raw):
    if num_docs == 100003:
        monkeypatch.setenv("PINOT_GPU_TEST_CUS", "1")                   # a grid sized for one CU: a wave walks many tiles
    seg = HL.edge_segment(S, num_docs, raw)
    n = num_docs
    f_lt = lambda t: Q.leaf(Q.Pred.dict_range(HL.E_FILTER, 0, t))
    with engine.open(seg) as g:
        def check(spec, where, match=None, kernel=None):
            got = g.execute(spec)
            HL.assert_registers_equal(got, seg, spec, where="%s n=%d %s" % ("raw" if raw else "dict", n, where), match=match)
            if kernel is not None:
                assert got.dominant_kernel == kernel, (where, got.dominant_kernel)
            return got

        # the four stored types at the default log2m: no filter (a dictionary column: the whole dictionary, nothing scanned), then behind a range leaf
        got = check(Q.QuerySpec(hll_specs(seg)), "no filter", kernel=SCAN_RAW if raw else None)
        assert got.stats == ((n, 0, 4 * n, n) if raw else (n, 0, 0, n)), got.stats
        check(Q.QuerySpec(hll_specs(seg) + [(Q.COUNT, -1)], filter=f_lt(500)), "range leaf", kernel=SCAN_RAW if raw else SCAN_DICT)
        # the smallest and the largest register count, behind a dictId set that is staged in LDS beside the registers
        in_list = Q.leaf(Q.Pred.dict_set(HL.E_SET, list(range(0, 300, 7)), 300))
        check(Q.QuerySpec([(Q.hll(4), HL.E_INT), (Q.hll(14), HL.E_DOUBLE), (Q.hll(14), HL.E_LONG), (Q.hll(4), HL.E_FLOAT)], filter=in_list), "log2m 4 / 14 behind a staged set")
        # no doc matches: all-zero registers, count 0
        got = check(Q.QuerySpec(hll_specs(seg), filter=Q.leaf(Q.Pred.match_none())), "no match")
        assert all(v.count == 0 and not np.any(v.hll_registers) for v in got.aggregations)
        # every doc carries one value: one non-zero register
        got = check(Q.QuerySpec([(Q.hll(), HL.E_ONE)], filter=f_lt(900)), "one value")
        if D.matching_docs(seg, Q.QuerySpec([], filter=f_lt(900))).any():
            assert got.aggregations[0].count == 1
        # a doc-set leaf (the oracle does not know doc sets: the model takes the mask)
        mask = np.random.default_rng(5).random(n) < 0.4
        doc_set = g.create_doc_set(doc_ids=np.flatnonzero(mask).astype(np.int32))
        check(Q.QuerySpec(hll_specs(seg, 12)[:2], filter=Q.leaf(Q.Pred.doc_set(doc_set))), "doc set", match=mask)
        g.release_doc_set(doc_set)
        # an index-led filter: the postings of one leaf list the tiles, the scan leaf runs over them
        led = Q.and_(Q.leaf(Q.Pred.dict_range(HL.E_FILTER, 100, 140, inverted=True)), Q.leaf(Q.Pred.dict_range(HL.E_SET, 0, 200)))
        check(Q.QuerySpec(hll_specs(seg), filter=led), "index-led")
        # GROUP BY with two keys
        two_keys = Q.QuerySpec(hll_specs(seg)[1:] + [(Q.COUNT, -1)], filter=f_lt(700), group_by=[HL.E_K1, HL.E_K2])
        got = check(two_keys, "two keys")
        pass_kernel_or_the_ordinary_one(g, two_keys, got, GROUP_RAW if raw else GROUP_DICT)
        assert got.group_id_upper_bound == 35
        check(Q.QuerySpec([(Q.hll(14), HL.E_FLOAT)], group_by=[HL.E_K2]), "one key, no filter, log2m 14")


# ---- 5. one bitset per column, whoever uses it ----
def test_a_column_shared_by_distinctcount_and_two_hlls(engine):
    seg = HL.edge_segment(S, 100003, raw=False)
    c = HL.E_LONG
    for group_by in ([], [HL.E_K1]):
        spec = Q.QuerySpec([(Q.DISTINCTCOUNT, c), (Q.hll(), c), (Q.hll(12), c), (Q.COUNT, -1)], filter=Q.leaf(Q.Pred.dict_range(HL.E_FILTER, 0, 300)), group_by=group_by)
        with engine.open(seg) as g:
            got = g.execute(spec)
        HL.assert_registers_equal(got, seg, spec)
        D.assert_sets_equal(got, seg, spec)
        rows = got.groups.values() if group_by else [got.aggregations]
        assert all(len(r[1].hll_registers) == 256 and len(r[2].hll_registers) == 4096 for r in rows)


# ---- 6. declines: the same status and message from pg_query_check and pg_execute ----
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


def test_declines_name_their_reason(engine):
    n = 2049
    rng = np.random.default_rng(23)
    raw_int = lambda name: S.Column.raw_typed(name, rng.integers(-1000, 1000, n).astype(np.int32))
    nullable = S.Column.raw_typed("rn", rng.integers(0, 50, n).astype(np.int32)).with_nulls(rng.random(n) < 0.2)
    cols = [raw_int("r0"), raw_int("r1"), raw_int("r2"), raw_int("r3"), raw_int("r4"),                                # 0-4
            S.Column.from_dict_ids("d", np.arange(100, dtype=np.int32), rng.integers(0, 100, n).astype(np.int32)),     # 5
            S.Column.raw_typed("rl", rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64)),                             # 6
            nullable,                                                                                                  # 7
            S.Column.from_dict_ids("k", np.arange(9, dtype=np.int32), rng.integers(0, 9, n).astype(np.int32))]         # 8
    seg = S.SegmentData("hll_declines", n, cols)
    U, I = _abi.PG_ERR_UNSUPPORTED, _abi.PG_ERR_INVALID_ARGUMENT
    with engine.open(seg) as g:
        answered(g, Q.QuerySpec([(Q.hll(), 0), (Q.hll(), 5)]), U, r"DISTINCTCOUNTHLL on raw column r0 and dictionary column d in one query")
        answered(g, Q.QuerySpec([(Q.hll(), 0), (Q.DISTINCTCOUNT, 1)]), U, r"collect pass is off|DISTINCTCOUNTHLL on raw column r0 beside a DISTINCTCOUNT")
        answered(g, Q.QuerySpec([(Q.hll(), 0), (Q.PERCENTILE, 5)]), U, r"PERCENTILE beside DISTINCTCOUNTHLL")
        answered(g, Q.QuerySpec([(Q.hll(), 5), (Q.PERCENTILE, 5)]), U, r"PERCENTILE beside DISTINCTCOUNTHLL")
        answered(g, Q.QuerySpec([(Q.hll(), 0)], filter=Q.leaf(Q.Pred.raw_range(6, -5, 5))), U, r"DISTINCTCOUNTHLL beside a range predicate on raw LONG / FLOAT / DOUBLE column rl")
        answered(g, Q.QuerySpec([(Q.hll(), 7)], null_handling=True), U, r"DISTINCTCOUNTHLL on column rn, which carries a null value vector, under null handling")
        g.execute(Q.QuerySpec([(Q.hll(), 7)]))                          # (without the option the null vector is not looked at)
        answered(g, Q.QuerySpec([(Q.hll(), c) for c in range(5)]), U, r"more than 4 DISTINCTCOUNTHLL columns")
        # four register sets of 2^14 words are 256 KiB: more LDS than a workgroup has
        answered(g, Q.QuerySpec([(Q.hll(14), c) for c in range(4)]), U, r"DISTINCTCOUNTHLL registers of 262144 bytes .* exceed the \d+ bytes of LDS")
        g.execute(Q.QuerySpec([(Q.hll(14), 0), (Q.hll(14), 1)]))
        # log2m outside [4, 14], or bits above the low byte on another function: not a query at all
        answered(g, Q.QuerySpec([(_abi.PG_AGG_HLL(3), 0)]), I, r"log2m 3: outside \[4, 14\]")
        answered(g, Q.QuerySpec([(_abi.PG_AGG_HLL(15), 5)]), I, r"log2m 15: outside \[4, 14\]")
        answered(g, Q.QuerySpec([(Q.SUM | (8 << 8), 5)]), I, r"sets bits above the function's byte")
    with engine.open(seg) as g:
        engine.reinit(PINOT_GPU_COLLECT="1")
        try:
            answered(g, Q.QuerySpec([(Q.hll(), 0), (Q.DISTINCTCOUNT, 1)]), U, r"DISTINCTCOUNTHLL on raw column r0 beside a DISTINCTCOUNT")
        finally:
            engine.reinit(PINOT_GPU_COLLECT=None)
    # register matrices above PG_HLL_GROUP_MAX_BYTES, from metadata alone: 60000 raw keys x 2^14 registers x 4 bytes = 3.9 GB
    big = S.SegmentData("hll_cap", n, [raw_int("v"), S.Column.from_dict_ids("k1", np.arange(300, dtype=np.int32), rng.integers(0, 300, n).astype(np.int32)),
                                       S.Column.from_dict_ids("k2", np.arange(200, dtype=np.int32), rng.integers(0, 200, n).astype(np.int32)),
                                       S.Column.from_dict_ids("dv", np.arange(50, dtype=np.int32), rng.integers(0, 50, n).astype(np.int32))])
    with engine.open(big) as g:
        before = g.device_bytes()
        answered(g, Q.QuerySpec([(Q.hll(14), 0)], group_by=[1, 2]), U, r"exceed PG_HLL_GROUP_MAX_BYTES")
        answered(g, Q.QuerySpec([(Q.hll(14), 3)], group_by=[1, 2]), U, r"exceed PG_HLL_GROUP_MAX_BYTES")
        assert g.device_bytes() == before                               # nothing was allocated


def test_the_accessor_rejects_what_is_not_a_sketch(engine):
    seg = HL.edge_segment(S, 2049, raw=True)
    spec = Q.QuerySpec([(Q.COUNT, -1), (Q.hll(), HL.E_INT)])
    with engine.open(seg) as g:
        res = _abi.pg_result()
        _abi.check(g.lib, g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res)))
        try:
            regs, num = C.POINTER(C.c_uint8)(), C.c_int32()
            call = lambda a, row: g.lib.pg_result_hll_registers(C.byref(res), a, row, C.byref(regs), C.byref(num))
            assert call(1, -1) == _abi.PG_OK and num.value == 256
            for a, row in ((0, -1), (2, -1), (-1, -1), (1, 0)):
                assert call(a, row) == _abi.PG_ERR_INVALID_ARGUMENT, (a, row)
        finally:
            g.lib.pg_result_free(C.byref(res))


# ---- 7. an HLL item of pg_execute_batch runs as a pg_execute of its own ----
def test_a_batch_with_hll_items_among_ordinary_ones(engine):
    raw_seg, dict_seg = HL.edge_segment(S, 2049, raw=True), HL.edge_segment(S, 2049, raw=False)
    flt = Q.leaf(Q.Pred.dict_range(HL.E_FILTER, 0, 600))
    ordinary = Q.QuerySpec([(Q.COUNT, -1)], filter=flt)
    hll = Q.QuerySpec(hll_specs(raw_seg), filter=flt)
    with engine.open(raw_seg) as gr, engine.open(dict_seg) as gd:
        out = engine.execute_batch([gr, gr, gd, gd], [ordinary, hll, hll, ordinary])
    assert [status for status, _ in out] == [_abi.PG_OK] * 4
    HL.assert_registers_equal(out[1][1], raw_seg, hll)
    HL.assert_registers_equal(out[2][1], dict_seg, hll)
    want = oracle.execute(raw_seg, ordinary)
    assert out[0][1].aggregations[0].count == want.aggregations[0].count == out[3][1].aggregations[0].count


# ---- 8. the JNI function over the accessor, executed through the JVM stand-in ----
def test_the_native_method_returns_the_registers_with_the_result(engine, goldens):
    from pinot_amd import jni_harness as J
    jvm = J.FakeJvm()
    jvm.call("init", None, C.c_int32(0), C.c_int32(0))
    try:
        refs_before = jvm.lib.fj_live_refs()
        for form in ("dict", "raw"):
            seg = goldens[form]
            ci = seg.column_index
            handle = jvm.segment_open(seg)
            try:
                for grouped in (False, True):
                    spec = Q.QuerySpec([(Q.COUNT, -1), (Q.hll(), ci("column1")), (Q.hll(), ci("column3"))], filter=H.golden_filter_physical(seg),
                                       group_by=[ci("column9")] if grouped else [])
                    assert jvm.query_check(handle, spec) == _abi.PG_OK
                    result, sketches = jvm.execute_with_hll_registers(handle, spec)
                    plain = jvm.execute(handle, spec)
                    assert all(np.array_equal(a, b) for a, b in zip(result[1:], plain[1:])) and list(result[0][:4]) == list(plain[0][:4])
                    want = goldens["models"][(True, grouped)]            # (aggregations 0 / 1 of the model are 1 / 2 here)
                    group_ids = [int(x) for x in result[1]] if grouped else [None]
                    rows = len(group_ids)
                    assert len(sketches) == 3 * rows and all(x is None for x in sketches[:rows])
                    for a in (1, 2):
                        for r, gid in enumerate(group_ids):
                            regs = sketches[a * rows + r]
                            assert regs.dtype == np.uint8 and np.array_equal(regs, want[gid][a - 1] if grouped else want[a - 1]), (form, grouped, a, gid)
                            assert result[2][r * 3 + a] == int(np.count_nonzero(regs))      # counts: the non-zero registers
                    if not grouped:
                        row = HL.GOLDEN_ROWS["filter"]
                        assert (HL.cardinality(sketches[1]), HL.cardinality(sketches[2])) == (row["v1"], row["v2"])
            finally:
                jvm.call("segmentClose", None, C.c_int64(handle))
        assert jvm.lib.fj_live_refs() == refs_before
    finally:
        engine.reinit()
