"""CPU tests of DISTINCTCOUNT: the model of tests/distinct_cases.py is pinned to the reference's own numbers
(InterSegmentAggregationSingleValueQueriesTest.testDistinctCount :235-258, over the committed fixture), the C header and its Python
mirror agree on the additions, and the host mirror parses the function, merges value sets by union through host.group_by_combine, gives the
size as the INT final result and orders by it."""
import os
import re

import numpy as np
import pytest

import distinct_cases as D
import helpers as H
from pinot_amd import _abi
from pinot_amd import host
from pinot_amd import query as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return H.golden_segment()


@pytest.mark.parametrize("row,filtered,grouped", [("plain", False, False), ("filter", True, False), ("group", False, True), ("filter+group", True, True)])
def test_the_model_reproduces_the_reference_rows(golden, row, filtered, grouped):
    seg = golden
    want = D.GOLDEN_ROWS[row]
    spec = D.golden_spec(seg, filtered, grouped)
    sets = D.model(seg, spec)
    docs = int(D.matching_docs(seg, spec).sum())
    assert docs == want["stats"][0]
    if not grouped:
        assert (len(sets[0]), len(sets[1])) == (want["v1"], want["v2"])
        return
    # ORDER BY v1 DESC, v2 DESC LIMIT 1
    top = max(sets, key=lambda g: (len(sets[g][0]), len(sets[g][1])))
    assert top == D.golden_group_id(seg)
    assert (len(sets[top][0]), len(sets[top][1])) == (want["v1"], want["v2"])
    assert docs * D.projected_columns(spec) == want["stats"][2]
    assert seg.columns[seg.column_index("column9")].cardinality == 1737


def test_the_filtered_rows_of_every_filter_form_are_the_same_docs(golden):
    seg = golden
    a = D.matching_docs(seg, D.golden_spec(seg, True, False, "logical"))
    for form in ("inverted", "physical"):
        assert np.array_equal(a, D.matching_docs(seg, D.golden_spec(seg, True, False, form)))


def test_the_header_and_its_mirror_agree_on_the_additions():
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+5\b", header) and _abi.PG_ABI_VERSION == 5
    assert re.search(r"\bPG_AGG_DISTINCTCOUNT\s*=\s*5\b", header) and _abi.PG_AGG_DISTINCTCOUNT == 5 == Q.DISTINCTCOUNT
    assert re.search(r"\bPG_KERNEL_SCAN_DISTINCT\s*=\s*14\b", header) and _abi.KERNEL_NAMES[14] == "scan_distinct_kernel"
    assert re.search(r"\bPG_KERNEL_GROUP_DISTINCT\s*=\s*15\b", header) and _abi.KERNEL_NAMES[15] == "group_distinct_kernel"
    assert re.search(r"#define\s+PG_DISTINCT_GROUP_MAX_BYTES\s+\(1ull << 30\)", header) and _abi.PG_DISTINCT_GROUP_MAX_BYTES == 1 << 30
    m = re.search(r"#define\s+PG_DISTINCT_LDS_MAX_DICT_IDS\s+(\d+)\b", header)
    assert m and int(m.group(1)) == _abi.PG_DISTINCT_LDS_MAX_DICT_IDS
    assert "pg_result_distinct_dict_ids" in header and any(name == "pg_result_distinct_dict_ids" for name, _, _ in _abi.ABI_SYMBOLS)
    assert "no struct layout changed, one enumerator and one function added" in header


def test_the_host_mirror_parses_both_spellings():
    q = host.parse_sql("SELECT DISTINCTCOUNT(column1) AS v1, DISTINCT_COUNT(column3) FROM testTable WHERE column1 > 100000000")
    assert q["aggregations"] == ["distinctcount(column1)", "distinctcount(column3)"] and q["hasFilter"]
    q = host.parse_sql("SELECT DISTINCTCOUNT(column1) AS v1, DISTINCTCOUNT(column3) AS v2 FROM testTable GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1")
    assert q["aggregations"] == ["distinctcount(column1)", "distinctcount(column3)"] and q["groupBy"] == ["column9"] and q["limit"] == 1
    assert [(o["expression"], o["asc"]) for o in q["orderBy"]] == [("distinctcount(column1)", False), ("distinctcount(column3)", False)]
    q = host.parse_sql("SELECT COUNT(*), DistinctCount(column1) FROM testTable GROUP BY column9 ORDER BY distinct_count(column1) DESC")
    assert q["aggregations"] == ["count(*)", "distinctcount(column1)"] and q["orderBy"][0]["expression"] == "distinctcount(column1)"


def test_count_distinct_raises():
    with pytest.raises(host.HostError) as e:
        host.parse_sql("SELECT COUNT(DISTINCT column1) FROM testTable")
    assert e.value.status in (1, 2)


# ---- the mirror's merge, through host.group_by_combine (GroupByCombineOperator + GroupByDataTableReducer, no device) ----
def _cell(values):
    return (0, 0.0, 0.0, 0.0, False, values)


def test_the_combine_unions_overlapping_value_sets_and_the_final_is_the_size():
    sql = "SELECT DISTINCTCOUNT(m1), COUNT(*) FROM t GROUP BY d1 LIMIT 10"
    count = lambda n: (n, 0.0, 0.0, 0.0, False)
    blocks = [[((1,), [_cell([5, 7, 9, -3]), count(4)]), ((2,), [_cell([100]), count(1)])],
              [((1,), [_cell([7, 9, 11, 2 ** 40]), count(5)]), ((3,), [_cell([]), count(0)])],
              [((2,), [_cell([100, 100, 101]), count(3)])]]
    out = host.group_by_combine(sql, blocks, [host.KEY_INT])
    groups = {tuple(g["key"]): g for g in out["combined"]["groups"]}
    assert groups[(1,)]["intermediate"][0] == {"values": [-3, 5, 7, 9, 11, 2 ** 40]} and groups[(1,)]["final"] == [6, 9]
    assert groups[(2,)]["intermediate"][0] == {"values": [100, 101]} and groups[(2,)]["final"] == [2, 4]
    assert groups[(3,)]["intermediate"][0] == {"values": []} and groups[(3,)]["final"] == [0, 0]
    assert sorted(map(tuple, out["reduced"])) == [(1, 6, 9), (2, 2, 4), (3, 0, 0)]
    assert all(isinstance(r[1], int) for r in out["reduced"])            # an INT final result


def test_order_by_the_final_desc_with_a_tie_broken_by_the_second_column():
    sql = "SELECT DISTINCTCOUNT(m1) AS v1, DISTINCTCOUNT(m2) AS v2 FROM t GROUP BY d1 ORDER BY v1 DESC, v2 DESC LIMIT 2"
    # per key, over two segments: d1 = 1 -> (3, 1), d1 = 2 -> (3, 2), d1 = 3 -> (2, 9): the sizes only exist after the union
    blocks = [[((1,), [_cell([1, 2]), _cell([8])]), ((2,), [_cell([1]), _cell([8])]), ((3,), [_cell([4, 5]), _cell(range(9))])],
              [((1,), [_cell([2, 3]), _cell([8])]), ((2,), [_cell([2, 3]), _cell([9])]), ((3,), [_cell([5]), _cell(range(5))])]]
    out = host.group_by_combine(sql, blocks, [host.KEY_INT])
    assert out["reduced"] == [[2, 3, 2], [1, 3, 1]]
    assert out["resultTable"]["rows"] == [[3, 2], [3, 1]]
    out = host.group_by_combine(sql.replace("LIMIT 2", "LIMIT 1").replace("v2 DESC", "v2 ASC"), blocks, [host.KEY_INT])
    assert out["resultTable"]["rows"] == [[3, 1]]
