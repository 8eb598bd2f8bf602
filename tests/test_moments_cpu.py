"""VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP without a device: the cases' own arithmetic, the header and its mirrors, the host mirror's parser,
combine and finals (ph_combine_moments).  The merged tuples are held bit for bit to the restated VarianceTuple.apply(VarianceTuple)."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import moments_cases as M
from pinot_amd import _abi
from pinot_amd import host
from pinot_amd import query as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


# ---- the cases: where the reference's own arithmetic stands against the exact model ----
def reference_error(name, n):
    doubles = M.as_doubles(M.family_values(name, n))
    count, total, m2 = M.reference_tuple(doubles)
    got_n, _, e, x_max = M.Exact(doubles).moments()
    assert count == got_n == n
    return abs(Fraction(m2) - e), M.tol(n, e, x_max), e


@pytest.mark.parametrize("name,n", [(name, M.BIG) for name in M.PARITY] + M.PARITY_SMALL)
def test_the_reference_stays_inside_the_tolerance_on_the_parity_families(name, n):
    error, bound, e = reference_error(name, n)
    print("%s n=%d: reference error %.3e, tol %.3e, E %.6e" % (name, n, float(error), float(bound), float(e)))
    assert error <= bound


@pytest.mark.parametrize("name", M.BEYOND)
def test_the_reference_leaves_the_tolerance_on_the_beyond_families(name):
    """These families are held against the exact model only: if the reference came inside the bound here, the cases would have gone soft."""
    error, bound, e = reference_error(name, M.BIG)
    print("%s: reference error %.3e, tol %.3e, E %.6e" % (name, float(error), float(bound), float(e)))
    assert error > bound


def test_a_pivoted_pass_in_any_order_stays_inside_the_tolerance():
    """The two-run scheme simulated in doubles, additions in a random order, the pivot carrying a plain running SUM's rounding."""
    rng = np.random.default_rng(3)
    for name in M.PARITY + M.BEYOND + ["int_full", "double_unit", "long_wide"]:
        doubles = M.as_doubles(M.family_values(name, M.BIG))
        n, _, e, x_max = M.Exact(doubles).moments()
        c = float(np.cumsum(doubles)[-1]) / n
        d = doubles[rng.permutation(n)] - c
        s1, s2 = float(np.cumsum(d)[-1]), float(np.cumsum(d * d)[-1])
        m2 = max(s2 - s1 * s1 / n, 0.0)
        assert abs(Fraction(m2) - e) <= M.tol(n, e, x_max), name


# ---- the header and its mirrors ----
def test_the_header_and_its_mirror_agree_on_the_additions():
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+5\b", header) and _abi.PG_ABI_VERSION == 5
    assert re.search(r"\bPG_AGG_VARIANCE\s*=\s*8\b", header) and _abi.PG_AGG_VARIANCE == 8 == Q.VARIANCE
    assert re.search(r"#define\s+PG_MOMENTS_GROUP_MAX_BYTES\s+\(1ull << 30\)", header) and _abi.PG_MOMENTS_GROUP_MAX_BYTES == 1 << 30
    assert re.search(r"\bPG_KERNEL_SCAN_MOMENTS\s*=\s*22\b", header) and _abi.KERNEL_NAMES[22] == "scan_moments_kernel"
    assert re.search(r"\bPG_KERNEL_GROUP_MOMENTS\s*=\s*23\b", header) and _abi.KERNEL_NAMES[23] == "group_moments_kernel"
    assert "pg_result_moments" in header and any(name == "pg_result_moments" for name, _, _ in _abi.ABI_SYMBOLS)


# ---- the parser ----
SPELLINGS = {"varpop": ["VAR_POP", "VARPOP", "var_pop", "VarPop"], "varsamp": ["VAR_SAMP", "VARSAMP", "var_samp"],
             "stddevpop": ["STDDEV_POP", "STD_DEV_POP", "STDDEVPOP", "stddev_pop"], "stddevsamp": ["STDDEV_SAMP", "STD_DEV_SAMP", "STDDEVSAMP", "StdDev_Samp"]}


def test_the_host_mirror_parses_every_spelling():
    for name, spellings in SPELLINGS.items():
        for spelling in spellings:
            q = host.parse_sql("SELECT %s(column1), COUNT(*) FROM testTable WHERE column1 > 5" % spelling)
            assert q["aggregations"] == ["%s(column1)" % name, "count(*)"] and q["hasFilter"], spelling
    q = host.parse_sql("SELECT STDDEV_POP(m) AS s, VAR_SAMP(m) FROM t GROUP BY d ORDER BY s DESC, var_samp(m) LIMIT 3")
    assert q["groupBy"] == ["d"] and q["limit"] == 3
    assert [(o["expression"], o["asc"]) for o in q["orderBy"]] == [("stddevpop(m)", False), ("varsamp(m)", True)]


def test_what_the_parser_declines():
    for sql, message in (("SELECT VARIANCE(column1) FROM testTable", r"DISTINCTCOUNTHLL/PERCENTILE are offloaded, got VARIANCE"),
                         ("SELECT COVAR_POP(column1, column3) FROM testTable", r"VARPOP/VARSAMP/STDDEVPOP/STDDEVSAMP/DISTINCTCOUNT/DISTINCTCOUNTHLL/PERCENTILE are offloaded, got COVAR_POP"),
                         ("SELECT SKEWNESS(column1) FROM testTable", r"DISTINCTCOUNTHLL/PERCENTILE are offloaded, got SKEWNESS"),
                         ("SELECT VAR_POP(*) FROM testTable", r"'\*' is only valid in COUNT\(\*\)"),
                         ("SELECT VAR_POP(column1, 2) FROM testTable", r"only identifier arguments are offloaded"),
                         ("SELECT VAR_POP(column1 + 1) FROM testTable", r"only identifier arguments are offloaded"),
                         ("SELECT COUNT(*) FROM testTable GROUP BY column9 ORDER BY STDDEV_POP(column1)", r"a STDDEVPOP that appears only in ORDER BY")):
        with pytest.raises(host.HostError) as e:
            host.parse_sql(sql)
        assert e.value.status in (1, 2), sql
        assert re.search(message, str(e.value)), (sql, str(e.value))


# ---- the combine, from host-supplied tuples (no device) ----
def _cell(t):
    return (t[0], t[1], 0.0, 0.0, False, t[2])


def _tuple_of(cell):
    return (cell["count"], float(cell["sum"]), float(cell["m2"]))


def block_tuples(name, blocks, n=5000):
    """The restated reference's tuple of every one of `blocks` equal slices of a family's values."""
    doubles = M.as_doubles(M.family_values(name, n))
    return [M.reference_tuple(part) for part in np.array_split(doubles, blocks)]


def bits(t):
    return (t[0], np.float64(t[1]).tobytes(), np.float64(t[2]).tobytes())


@pytest.mark.parametrize("blocks", [1, 2, 5])
def test_the_merged_tuple_is_the_references_bit_for_bit(blocks):
    for name in ("double_pm1e6", "long_1p7e12", "float_normal", "long_2p62"):
        tuples = block_tuples(name, blocks)
        out = host.combine_moments("SELECT VAR_POP(m), STDDEV_SAMP(m) FROM t", [[((), [_cell(t), _cell(t)])] for t in tuples])
        want = M.merge_tuples(tuples)
        for a in range(2):
            assert bits(_tuple_of(out["combined"]["intermediate"][a])) == bits(want), (name, blocks, a)
        assert out["combined"]["columns"] == ["varpop(m)", "stddevsamp(m)"]
        assert out["combined"]["final"] == [M.final("varpop", want), M.final("stddevsamp", want)]


@pytest.mark.parametrize("blocks", [1, 2, 5])
def test_the_merged_tuples_of_a_group_by_are_the_references_bit_for_bit(blocks):
    per_key = {key: block_tuples(name, blocks, 3000 + key) for key, name in ((1, "double_pm1e6"), (2, "int_uniform"), (7, "long_2p62"))}
    segments = [[((key,), [_cell(tuples[b])]) for key, tuples in per_key.items() if not (key == 2 and b == 1)] for b in range(blocks)]
    out = host.combine_moments("SELECT VAR_SAMP(m) FROM t GROUP BY d LIMIT 10", segments, [host.KEY_INT])
    groups = {g["key"][0]: g for g in out["combined"]["groups"]}
    assert sorted(groups) == [1, 2, 7]
    for key, tuples in per_key.items():
        want = M.merge_tuples([t for b, t in enumerate(tuples) if not (key == 2 and b == 1)])
        assert bits(_tuple_of(groups[key]["intermediate"][0])) == bits(want), key
        assert groups[key]["final"] == [M.final("varsamp", want)]


def test_an_empty_tuple_on_either_side_of_the_merge():
    t = (3, 6.0, 2.0)
    for blocks in ([(0, 0.0, 0.0), t], [t, (0, 0.0, 0.0)]):
        out = host.combine_moments("SELECT VAR_POP(m) FROM t", [[((), [_cell(b)])] for b in blocks])
        assert bits(_tuple_of(out["combined"]["intermediate"][0])) == bits(M.merge_tuples(blocks)) == bits(t)
    # under null handling a null side gives way to the other (merge :158-166)
    sql = "SET enableNullHandling = true; SELECT VAR_POP(m) FROM t"
    out = host.combine_moments(sql, [[((), [(0, 0.0, 0.0, 0.0, True, 0.0)])], [((), [_cell(t)])]])
    assert bits(_tuple_of(out["combined"]["intermediate"][0])) == bits(t)
    out = host.combine_moments(sql, [[((), [(0, 0.0, 0.0, 0.0, True, 0.0)])], [((), [(0, 0.0, 0.0, 0.0, True, 0.0)])]])
    assert out["combined"]["intermediate"] == [None] and out["combined"]["final"] == [None]


def test_the_finals_of_no_doc_one_doc_and_two_docs():
    sql = "SELECT VAR_POP(m), VAR_SAMP(m), STDDEV_POP(m), STDDEV_SAMP(m) FROM t"
    kinds = ("varpop", "varsamp", "stddevpop", "stddevsamp")
    for t, want in (((0, 0.0, 0.0), [-INF, -INF, -INF, -INF]), ((1, 5.0, 0.0), [0.0, -INF, 0.0, -INF]),
                    ((2, 4.0, 2.0), [1.0, 2.0, 1.0, math.sqrt(2.0)])):
        out = host.combine_moments(sql, [[((), [_cell(t)] * 4)]])
        final = [float(x) for x in out["combined"]["final"]]            # (the JSON spells -inf as a string)
        assert final == want == [M.final(kind, t) for kind in kinds], t


def test_order_by_a_standard_deviation():
    sql = "SELECT STDDEV_POP(m) AS s FROM t GROUP BY d ORDER BY s DESC LIMIT 2"
    cells = {1: (4, 8.0, 4.0), 2: (4, 8.0, 100.0), 3: (0, 0.0, 0.0), 4: (2, 1.0, 50.0)}
    out = host.combine_moments(sql, [[((key,), [_cell(t)]) for key, t in cells.items()]], [host.KEY_INT])
    assert out["reduced"] == [[2, 5.0], [4, 5.0]] or out["reduced"] == [[4, 5.0], [2, 5.0]]
    out = host.combine_moments("SELECT STDDEV_POP(m) AS s FROM t GROUP BY d ORDER BY s LIMIT 2", [[((key,), [_cell(t)]) for key, t in cells.items()]], [host.KEY_INT])
    assert [row[0] for row in out["reduced"]] == [3, 1] and float(out["reduced"][0][1]) == -INF and out["reduced"][1][1] == 1.0


def test_query_spec_carries_the_function():
    spec = Q.QuerySpec([(Q.VARIANCE, 3), (Q.COUNT, -1)])
    assert spec.c.aggregations[0].function == 8 and spec.c.aggregations[0].column == 3
