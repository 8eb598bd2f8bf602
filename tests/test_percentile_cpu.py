"""CPU tests of PERCENTILE: the C header and its Python mirror agree on the additions; the host mirror parses the reference's three spellings
and declines the others; its value list (ValueCounts: ascending runs of (value, count)) merges and gives the final result of
PercentileAggregationFunction.extractFinalResult (:155-172) -- held against a brute-force sort; and the reference's sixteen testPercentile
doubles (InterSegmentAggregationSingleValueQueriesTest :379-473) come out of the committed fixture through the host-only combine
(host.combine_counts), fed the counts of the numpy model of tests/percentile_cases.py."""
import os
import re

import numpy as np
import pytest

import helpers as H
import percentile_cases as P
from pinot_amd import _abi
from pinot_amd import host
from pinot_amd import query as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_and_its_mirror_agree_on_the_additions():
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+5\b", header) and _abi.PG_ABI_VERSION == 5
    assert re.search(r"\bPG_AGG_PERCENTILE\s*=\s*6\b", header) and _abi.PG_AGG_PERCENTILE == 6 == Q.PERCENTILE
    assert re.search(r"\bPG_KERNEL_SCAN_COUNTS\s*=\s*16\b", header) and _abi.KERNEL_NAMES[16] == "scan_counts_kernel"
    assert re.search(r"\bPG_KERNEL_GROUP_COUNTS\s*=\s*17\b", header) and _abi.KERNEL_NAMES[17] == "group_counts_kernel"
    assert re.search(r"#define\s+PG_PERCENTILE_GROUP_MAX_BYTES\s+\(1ull << 30\)", header) and _abi.PG_PERCENTILE_GROUP_MAX_BYTES == 1 << 30
    m = re.search(r"#define\s+PG_PERCENTILE_LDS_MAX_COUNTERS\s+(\d+)\b", header)
    assert m and int(m.group(1)) == _abi.PG_PERCENTILE_LDS_MAX_COUNTERS
    assert "pg_result_percentile_counts" in header and any(name == "pg_result_percentile_counts" for name, _, _ in _abi.ABI_SYMBOLS)
    assert "(still 5) PG_AGG_PERCENTILE, pg_result_percentile_counts: no struct layout changed, one enumerator and one function added" in header


def test_the_slack_behind_the_last_counter_is_part_of_the_byte_arithmetic():
    """plan_percentile's sizing rule, from the source: group_id_upper_bound x cardinality x 4 bytes per column plus 2^bits - cardinality (+ 1)
    counters behind the last one -- what a dictId beyond the dictionary's bound could reach.  (tests/test_gpu_percentile.py holds the
    engine's message to this sum; no test provokes a stray write.)"""
    layout = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_set_pass_layout.h")).read()
    body = layout[layout.index("inline size_t counts_slack_words"):]
    body = body[:body.index("}") + 1]
    assert "(size_t)1 << bits" in body and "by_width - by_card" in body and "+ 1" in body
    # the matrix total is rows x row words + the largest slack, and a counter row's slack is counts_slack_words
    total = layout[layout.index("struct SetMatrixLayout"):layout.index("// DISTINCTCOUNTHLL.")]
    assert "set_slack_words(counters, bits, cardinality)" in total and "return row_words + slack_words;" in total
    assert "counters ? counts_slack_words(bits, cardinality)" in layout
    engine = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_engine.hip")).read()
    plan = engine[engine.index("static pg_status plan_percentile"):engine.index("static pg_status execute_percentile")]
    assert "counters.add(true, product," in plan and "counters.total_words() * 4ull" in plan and "PG_PERCENTILE_GROUP_MAX_BYTES" in plan and "group_table_bytes" in plan


# ---- the SQL forms ----
def test_the_host_mirror_parses_the_three_spellings():
    q = host.parse_sql("SELECT PERCENTILE50(column1) AS v1, PERCENTILE99(column3) AS v2 FROM testTable WHERE column1 > 100000000")
    assert q["aggregations"] == ["percentile50(column1)", "percentile99(column3)"] and q["hasFilter"]
    q = host.parse_sql("SELECT PERCENTILE(column1, 50) AS v1, PERCENTILE(column3, '50') AS v2, percentile(column3, 99.9) FROM testTable")
    assert q["aggregations"] == ["percentile(column1, 50.0)", "percentile(column3, 50.0)", "percentile(column3, 99.9)"]
    q = host.parse_sql("SELECT PERCENTILE90(column1) AS v1, PERCENTILE(column3, 90) AS v2 FROM testTable GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1")
    assert q["aggregations"] == ["percentile90(column1)", "percentile(column3, 90.0)"] and q["groupBy"] == ["column9"] and q["limit"] == 1
    assert [(o["expression"], o["asc"]) for o in q["orderBy"]] == [("percentile90(column1)", False), ("percentile(column3, 90.0)", False)]
    assert host.parse_sql("SELECT PERCENTILE0(c), PERCENTILE100(c), PERCENTILE(c, 0), PERCENTILE(c, 100.0) FROM t")["aggregations"] == [
        "percentile0(c)", "percentile100(c)", "percentile(c, 0.0)", "percentile(c, 100.0)"]


@pytest.mark.parametrize("sql", ["SELECT PERCENTILE(c, 100.5) FROM t", "SELECT PERCENTILE(c, -1) FROM t", "SELECT PERCENTILE101(c) FROM t", "SELECT PERCENTILE(c) FROM t",
                                 "SELECT PERCENTILE(c, 'abc') FROM t"])
def test_a_percentile_outside_0_100_is_a_query_exception(sql):
    with pytest.raises(host.HostError) as e:
        host.parse_sql(sql)
    assert e.value.status == 1, str(e.value)


@pytest.mark.parametrize("name", ["PERCENTILEEST50", "PERCENTILETDIGEST99", "PERCENTILEKLL", "PERCENTILERAWEST50", "PERCENTILERAWTDIGEST90", "PERCENTILE50MV",
                                  "PERCENTILESMARTTDIGEST", "PERCENTILERAWKLL", "PERCENTILE_TDIGEST"])
def test_the_other_percentile_spellings_stay_declined(name):
    args = "(c, 50)" if name in ("PERCENTILEKLL", "PERCENTILESMARTTDIGEST", "PERCENTILERAWKLL", "PERCENTILE_TDIGEST") else "(c)"
    with pytest.raises(host.HostError) as e:
        host.parse_sql("SELECT %s%s FROM t" % (name, args))
    assert e.value.status == 1 and "not offloaded" in str(e.value)


# ---- the value list: merge and final result against a brute-force sort ----
def brute_force(values, p):
    """PercentileAggregationFunction.extractFinalResult on the expanded list."""
    if len(values) == 0:
        return float("-inf")
    s = np.sort(np.asarray(values, dtype=np.float64))
    return float(s[-1] if p == 100 else s[int(float(len(s)) * p / 100.0)])


def runs(values):
    v, n = np.unique(np.asarray(values, dtype=np.float64), return_counts=True)
    return v, n


def cell(values):
    return (len(values), 0.0, 0.0, 0.0, False, runs(values))


def name_of(p):
    return "PERCENTILE%d(m)" % p if float(p).is_integer() else "PERCENTILE(m, %r)" % p


@pytest.mark.parametrize("length", [1, 2, 3, 1000])
def test_merge_and_final_result_equal_a_brute_force_sort(length):
    rng = np.random.default_rng(length)
    ps = [0, 50, 99, 99.9, 100]
    sql = "SELECT %s FROM t" % ", ".join(name_of(p) for p in ps)
    for trial in range(4):
        values = rng.integers(-50, 50, length).astype(np.float64) * 1.5
        # one segment, and the same list split over three segments (one of them possibly empty): the merge is addAll up to order
        cuts = sorted(rng.integers(0, length + 1, 2))
        parts = [values[:cuts[0]], values[cuts[0]:cuts[1]], values[cuts[1]:]]
        for blocks in ([values], parts):
            out = host.combine_counts(sql, [[((), [cell(part)] * len(ps))] for part in blocks])
            want = [brute_force(values, p) for p in ps]
            assert out["combined"]["final"] == want, (length, trial, out["combined"]["final"], want)
            v, n = runs(values)
            assert out["combined"]["intermediate"][0] == {"values": list(v), "counts": [int(x) for x in n]}


def test_the_index_is_long_times_double_truncated():
    # size 1000, p 99.9 -> 999.0000000000001 -> 999; size 3, p 50 -> 1; size 2, p 50 -> 1; p 100 -> the last value, not values[size]
    assert [P.percentile_index(1000, 99.9), P.percentile_index(3, 50), P.percentile_index(2, 50), P.percentile_index(7, 100), P.percentile_index(1, 0)] == [999, 1, 1, 6, 0]
    values = np.arange(1000, dtype=np.float64)
    out = host.combine_counts("SELECT PERCENTILE(m, 99.9), PERCENTILE(m, 29), PERCENTILE100(m) FROM t", [[((), [cell(values)] * 3)]])
    assert out["combined"]["final"] == [999.0, float(int(1000.0 * 29 / 100.0)), 999.0]


def test_the_empty_list():
    empty = (0, 0.0, 0.0, 0.0, False, (np.zeros(0), np.zeros(0, np.int64)))
    out = host.combine_counts("SELECT PERCENTILE50(m), PERCENTILE(m, 99) FROM t", [[((), [empty, empty])], [((), [empty, empty])]])
    assert out["combined"]["final"] == ["-Infinity", "-Infinity"] and out["combined"]["intermediate"][0] == {"values": [], "counts": []}
    # under null handling a holder no value reached is null, and so is the final result
    null = (0, 0.0, 0.0, 0.0, True, (np.zeros(0), np.zeros(0, np.int64)))
    out = host.combine_counts("SET enableNullHandling = true; SELECT PERCENTILE50(m) FROM t", [[((), [null])], [((), [null])]])
    assert out["combined"]["final"] == [None] and out["combined"]["intermediate"] == [None]
    # ... and merges as the other side
    out = host.combine_counts("SET enableNullHandling = true; SELECT PERCENTILE50(m) FROM t", [[((), [null])], [((), [cell([4.0, 2.0, 9.0])])]])
    assert out["combined"]["final"] == [4.0]


def test_two_longs_that_share_a_double_become_one_run():
    a, b = 2 ** 53, 2 ** 53 + 1
    assert a != b and float(a) == float(b)
    both = (np.asarray([float(a), float(b), 5.0]), np.asarray([2, 3, 1], dtype=np.int64))          # runs as a LONG dictionary would give them
    out = host.combine_counts("SELECT PERCENTILE50(m) FROM t", [[((), [(6, 0.0, 0.0, 0.0, False, both)])]])
    assert out["combined"]["intermediate"][0] == {"values": [5.0, float(a)], "counts": [1, 5]} and out["combined"]["final"] == [float(a)]


def test_order_by_the_final_double():
    sql = "SELECT PERCENTILE50(m1) AS v1, PERCENTILE(m2, 90) AS v2 FROM t GROUP BY d1 ORDER BY v1 DESC, v2 DESC LIMIT 2"
    # per key over two segments -- the finals only exist after the merge: d1 = 1 -> (5, 8), d1 = 2 -> (5, 9), d1 = 3 -> (4, 100)
    blocks = [[((1,), [cell([1, 5]), cell([8])]), ((2,), [cell([5]), cell([9])]), ((3,), [cell([4, 4]), cell([100])])],
              [((1,), [cell([5, 9]), cell([8])]), ((2,), [cell([1, 7, 5]), cell([9])]), ((3,), [cell([9]), cell([100])])]]
    out = host.combine_counts(sql, blocks, [host.KEY_INT])
    assert out["reduced"] == [[2, 5.0, 9.0], [1, 5.0, 8.0]]
    assert out["resultTable"]["rows"] == [[5.0, 9.0], [5.0, 8.0]]


# ---- the reference's sixteen goldens, from the fixture through the host-only combine ----
@pytest.fixture(scope="module")
def golden():
    seg = H.golden_segment()
    return seg, {shape: P.model(seg, P.golden_spec(seg, *P.GOLDEN_SHAPES[shape])) for shape in P.GOLDEN_SHAPES}


def golden_cell(seg, column, pairs):
    ids, counts = pairs
    return (int(counts.astype(np.int64).sum()), 0.0, 0.0, 0.0, False, (P.values_of(seg, seg.column_index(column), ids), counts.astype(np.int64)))


@pytest.mark.parametrize("p", [50, 90, 95, 99])
@pytest.mark.parametrize("shape", ["plain", "filter", "group", "filter+group"])
def test_the_sixteen_goldens_from_the_fixture_through_the_combine(golden, shape, p):
    seg, models = golden
    lists = models[shape]
    grouped = P.GOLDEN_SHAPES[shape][1]
    spellings = ["SELECT PERCENTILE%d(column1) AS v1, PERCENTILE%d(column3) AS v2 FROM testTable" % (p, p)]
    if p == 50:
        spellings += ["SELECT PERCENTILE(column1, 50) AS v1, PERCENTILE(column3, 50) AS v2 FROM testTable",
                      "SELECT PERCENTILE(column1, '50') AS v1, PERCENTILE(column3, '50') AS v2 FROM testTable"]
    if grouped:
        c9 = seg.columns[seg.column_index("column9")]
        block = [((int(c9.value_of(gid)),), [golden_cell(seg, "column1", l[0]), golden_cell(seg, "column3", l[1])]) for gid, l in sorted(lists.items())]
    else:
        block = [((), [golden_cell(seg, "column1", lists[0]), golden_cell(seg, "column3", lists[1])])]
    assert sum(cells[0][0] for _, cells in block) == P.GOLDEN_STATS[shape][0]          # the docs of one segment
    for sql in spellings:
        if grouped:
            out = host.combine_counts(sql + " GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1", [block] * 4, [host.KEY_INT])
            assert out["resultTable"]["rows"] == [list(P.GOLDEN_VALUES[(p, shape)])], sql
        else:
            out = host.combine_counts(sql, [block] * 4)
            assert out["combined"]["final"] == list(P.GOLDEN_VALUES[(p, shape)]), sql
