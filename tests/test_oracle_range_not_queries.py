"""RangeQueriesTest / NotOperatorQueriesTest pinned on the CPU tier: the rows are built from the reference tests' formulas, every golden of
tests/golden/range_queries_kats.json and not_operator_kats.json is checked against the oracle, with the predicates lowered by the product's own
C++ planner (FilterPlanNode mirror: `explain_filter`) and, for the raw FLOAT / DOUBLE columns, by its raw range evaluator
(RangePredicateEvaluatorFactory.newRawValueBasedEvaluator mirror) -- the bounds are never written by the test.

The GPU tier (test_gpu_range_not_queries.py) runs the same goldens through SQL on the device and imports the builders below."""
import ctypes as C
import json
import os
import re
import struct

import numpy as np
import pytest

import helpers as H
from oracle import oracle
from pinot_amd import host
from pinot_amd import query as Q
from pinot_amd import segment as S

RANGE_KATS = json.load(open(os.path.join(H.GOLDEN_DIR, "range_queries_kats.json")))
NOT_KATS = json.load(open(os.path.join(H.GOLDEN_DIR, "not_operator_kats.json")))
RANGE_COLS = ["dictionarizedIntCol", "rawIntCol", "rawLongCol", "rawFloatCol", "rawDoubleCol"]
RAW_TYPE = {"rawIntCol": 0, "rawLongCol": 1, "rawFloatCol": 2, "rawDoubleCol": 3}      # ph_lower_raw_range_predicate data types
RANGE_PERIOD = 1000           # RangeQueriesTest's values repeat every NUM_RECORDS rows
NOT_PERIOD = 1024             # NotOperatorQueriesTest: FIRST_INT_COL = i, so its goldens hold for the first 1 024 docs only


def range_values(n):
    """RangeQueriesTest.java:108: intValue = ((MAX_VALUE + NUM_RECORDS / 2) - (i * 100)) % MAX_VALUE, repeated every 1 000 rows past 1 000."""
    i = np.arange(n, dtype=np.int64) % RANGE_PERIOD
    return ((100_000 + 500) - i * 100) % 100_000


def range_segment(n=RANGE_PERIOD, raw_int_dictionary=False, name="testSegment"):
    """dictionarizedIntCol (dictionary) + rawIntCol / rawLongCol / rawFloatCol / rawDoubleCol (no dictionary, setNoDictionaryColumns).
    raw_int_dictionary: the reference's "after reload" variant with a dictionary on rawIntCol."""
    v = range_values(n)
    v32 = v.astype(np.int32)
    raw_int = S.Column.dict_encoded("rawIntCol", v32) if raw_int_dictionary else S.Column.raw("rawIntCol", v32)
    return S.SegmentData(name, n, [S.Column.dict_encoded("dictionarizedIntCol", v32), raw_int, S.Column.raw_typed("rawLongCol", v.astype(np.int64)),
                                   S.Column.raw_typed("rawFloatCol", v.astype(np.float32)), S.Column.raw_typed("rawDoubleCol", v.astype(np.float64))])


def not_segment(n=NOT_PERIOD, name="testSegment"):
    """NotOperatorQueriesTest.java:101-113: FIRST_INT_COL = i, SECOND_INT_COL = 1000 + i, DOMAIN_NAMES = domainNames[i % 16].
    Both INT columns come out sorted (the segment creator's sorted index); DOMAIN_NAMES carries dictIds into the sorted string dictionary."""
    i = np.arange(n, dtype=np.int32)
    names = NOT_KATS["domain_names"]
    sorted_names = sorted(names)
    ids = np.array([sorted_names.index(s) for s in names], dtype=np.int32)[i % len(names)]
    seg = S.SegmentData(name, n, [S.Column.dict_encoded("FIRST_INT_COL", i), S.Column.dict_encoded("SECOND_INT_COL", 1000 + i),
                                  S.Column.from_dict_ids("DOMAIN_NAMES", np.arange(len(names), dtype=np.int32), ids)])
    seg.string_dicts = {"DOMAIN_NAMES": sorted_names}
    return seg


def like_dict_set(seg, case):
    """The LIKE / REGEXP_LIKE goldens lowered by hand (the SQL subset has no LIKE): the dictIds of the 16 domain names the pattern matches, as an
    exclusive set leaf.  LIKE is the anchored regex with % -> .* and _ -> . (RegexpPatternConverterUtils.likeToRegexpLike); REGEXP_LIKE is an
    unanchored find (RegexpLikePredicateEvaluatorFactory)."""
    f = case["filter"]
    m = re.fullmatch(r"DOMAIN_NAMES NOT LIKE '(.*)'", f)
    if m:
        rx = "".join(".*" if ch == "%" else "." if ch == "_" else re.escape(ch) for ch in m.group(1))
        match = lambda s: re.fullmatch(rx, s) is not None
    else:
        m = re.fullmatch(r"NOT REGEXP_LIKE\(DOMAIN_NAMES, '(.*)'\)", f)
        assert m, f
        match = lambda s: re.search(m.group(1), s) is not None
    names = seg.string_dicts["DOMAIN_NAMES"]
    ids = [d for d, s in enumerate(names) if match(s)]
    return Q.leaf(Q.Pred.dict_set(seg.column_index("DOMAIN_NAMES"), ids, len(names), exclusive=True))


def lower_raw(data_type, lower, lower_inclusive, upper, upper_inclusive):
    """ph_lower_raw_range_predicate: the product's raw range evaluator; FLOAT / DOUBLE bounds come back as the double bit patterns the ABI carries."""
    lib = host._lib()
    lib.ph_lower_raw_range_predicate.restype = C.c_void_p
    lib.ph_lower_raw_range_predicate.argtypes = [C.c_int32, C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]
    st = C.c_int32()
    ptr = lib.ph_lower_raw_range_predicate(data_type, str(lower).encode(), int(lower_inclusive), str(upper).encode(), int(upper_inclusive), C.byref(st))
    return host._take_json(lib, ptr, st)


def bits_to_f64(b):
    return struct.unpack("<d", struct.pack("<q", int(b)))[0]


_EXPLAIN_LEAF = re.compile(r"(SORTED|SCAN|INVERTED)\((\w+)( NOT)? (docs|raw|dictIds) (-?\d+)\.\.(-?\d+)\)")


def plan_of(seg, hseg, sql):
    """The filter tree the C++ planner builds for `sql` (explain_filter), rebuilt as a QuerySpec filter: the oracle then runs the product's own
    lowering -- sorted doc ranges, dictId ranges, raw bounds as bit patterns."""
    text = host.explain_filter(hseg, sql)
    pos = 0

    def node():
        nonlocal pos
        for const, make in (("MATCH_ALL", Q.Pred.match_all), ("EMPTY", Q.Pred.match_none)):
            if text.startswith(const, pos):
                pos += len(const)
                return Q.leaf(make())
        for op, make in (("NOT(", Q.not_), ("AND(", Q.and_), ("OR(", Q.or_)):
            if text.startswith(op, pos):
                pos += len(op)
                kids = [node()]
                while text.startswith(", ", pos):
                    pos += 2
                    kids.append(node())
                assert text[pos] == ")", text
                pos += 1
                return make(*kids)
        m = _EXPLAIN_LEAF.match(text, pos)
        assert m, (text, pos)
        pos = m.end()
        kind, col, neg, what, lo, hi = m.group(1), m.group(2), m.group(3) is not None, m.group(4), int(m.group(5)), int(m.group(6))
        ci = seg.column_index(col)
        if what == "docs":
            return Q.leaf(Q.Pred.doc_range(lo, hi, exclusive=neg))
        if what == "raw":
            return Q.leaf(Q.Pred(Q._abi.PG_PRED_RAW_RANGE, ci, lo, hi, exclusive=neg))
        return Q.leaf(Q.Pred.dict_range(ci, lo, hi + 1, exclusive=neg, inverted=kind == "INVERTED"))

    tree = node()
    assert pos == len(text), text
    return text, tree


def hand_lowered(seg, case):
    """A RangeQueriesTest count case lowered leaf by leaf: the dictionary column through H.range_pred / H.eq_pred, the raw columns through the
    product's raw evaluator (one merged range, what MergeRangeFilterOptimizer makes of `c > a and c < b`)."""
    col, lo, hi, incl = case["column"], case["min"], case["max"], case["inclusive"]
    is_eq = " = " in case["sql"]
    if col == "dictionarizedIntCol" or seg.column(col).dictionary is not None:
        if is_eq:
            return Q.leaf(H.eq_pred(seg, col, lo))
        return Q.leaf(H.range_pred(seg, col, lo, hi, incl, incl))
    dt = RAW_TYPE[col]
    lit = (lambda v: "%.1f" % v) if dt >= 2 else str
    ev = lower_raw(dt, lit(lo), incl, lit(hi), incl)
    if ev["alwaysFalse"]:
        return Q.leaf(Q.Pred.match_none())
    return Q.leaf(Q.Pred(Q._abi.PG_PRED_RAW_RANGE, seg.column_index(col), ev["rawLower"], ev["rawUpper"]))


def selection_mask(values, case):
    lo, hi = case["min"], case["max"]
    return (values >= lo) & (values <= hi) if case["inclusive"] else (values > lo) & (values < hi)


def count_spec(flt):
    return Q.QuerySpec([(Q.COUNT, -1)], filter=flt)


# ---------------------------------------------------------------------------------------------------------------------------------------
def test_fixtures_are_the_reference_cases():
    counts, sels = RANGE_KATS["count_cases"], RANGE_KATS["selection_cases"]
    assert len(counts) == 40 and len(sels) == 40 and len(NOT_KATS["cases"]) == 19 and NOT_KATS["broker_factor"] == 4
    for c, s in zip(counts, sels):
        assert (c["column"], c["min"], c["max"], c["inclusive"]) == (s["column"], s["min"], s["max"], s["inclusive"])
        assert s["sql"] == c["sql"].replace("select count(*)", "select rawIntCol")
        fp = c["column"] in ("rawFloatCol", "rawDoubleCol")
        lit = (lambda v: "%.1f" % v) if fp else str
        if " = " in c["sql"]:
            assert c["sql"].endswith("where %s = %s" % (c["column"], lit(c["min"])))
        elif c["inclusive"]:
            assert c["sql"].endswith("where %s between %s and %s" % (c["column"], lit(c["min"]), lit(c["max"])))
        else:
            assert c["sql"].endswith("where %s > %s and %s < %s" % (c["column"], lit(c["min"]), c["column"], lit(c["max"])))


@pytest.mark.parametrize("raw_int_dictionary", [False, True])
def test_range_count_goldens_on_the_oracle(raw_int_dictionary):
    seg = range_segment(raw_int_dictionary=raw_int_dictionary)
    hseg = host.HostSegment(seg, load=False)
    v = range_values(RANGE_PERIOD)
    try:
        for case in RANGE_KATS["count_cases"]:
            text, planned = plan_of(seg, hseg, case["sql"])
            got = oracle.execute(seg, count_spec(planned)).aggregations[0].count
            assert got == case["count"], (case, text)
            assert oracle.execute(seg, count_spec(hand_lowered(seg, case))).aggregations[0].count == case["count"], case
            assert int(selection_mask(v, case).sum()) == case["count"], case
            col = case["column"]
            if col in ("rawFloatCol", "rawDoubleCol"):
                # SCAN raw with the bounds' bit patterns: FLOAT literals parsed as float, exclusive bounds stepped in the column's precision
                t = np.float32 if col == "rawFloatCol" else np.float64
                lo, hi = t(case["min"]), t(case["max"])
                if " = " in case["sql"]:
                    want = "SCAN(%s raw %d..%d)" % (col, Q.f64_bits(lo), Q.f64_bits(lo))
                elif case["inclusive"]:
                    want = "SCAN(%s raw %d..%d)" % (col, Q.f64_bits(lo), Q.f64_bits(hi))
                else:
                    up, down = np.nextafter(lo, t(np.inf)), np.nextafter(hi, t(-np.inf))
                    want = "AND(SCAN(%s raw %d..%d), SCAN(%s raw %d..%d))" % (col, Q.f64_bits(up), Q.f64_bits(np.inf), col, Q.f64_bits(-np.inf), Q.f64_bits(down))
                assert text == want, (case, text)
            elif col != "dictionarizedIntCol" and not (col == "rawIntCol" and raw_int_dictionary):
                assert text.startswith("SCAN(%s raw " % col) or text.startswith("AND(SCAN(%s raw " % col), (case, text)
    finally:
        hseg.destroy()


def test_range_selection_goldens_on_the_oracle():
    """testSelectionOverRangeFilter: the selected rows are exactly the docs whose rawIntCol value satisfies (min, max, inclusive), and as many as
    the count golden of the same filter."""
    seg = range_segment()
    hseg = host.HostSegment(seg, load=False)
    v = range_values(RANGE_PERIOD)
    try:
        for case, count in zip(RANGE_KATS["selection_cases"], RANGE_KATS["count_cases"]):
            # (the SQL subset offloads aggregations only: the selection's WHERE clause is planned inside its COUNT(*) twin)
            _, planned = plan_of(seg, hseg, case["sql"].replace("select rawIntCol", "select count(*)"))
            words, card = oracle.filter_bitmap(seg, count_spec(planned))
            assert card == count["count"], case
            bits = np.unpackbits(np.asarray(words, dtype="<u8").view(np.uint8), bitorder="little")[:RANGE_PERIOD].astype(bool)
            assert np.array_equal(bits, selection_mask(v, case)), case
            assert int(bits.sum()) == count["count"], case
    finally:
        hseg.destroy()


def test_not_operator_goldens_on_the_oracle():
    seg = not_segment()
    hseg = host.HostSegment(seg, string_dicts=seg.string_dicts, load=False)
    try:
        for case in NOT_KATS["cases"]:
            if case["group"] == "like":
                flt = like_dict_set(seg, case)
            else:
                text, flt = plan_of(seg, hseg, NOT_KATS["query"].replace("<filter>", case["filter"]))
                # SortedIndexBasedFilterOperator for both sorted INT columns: nothing is scanned
                assert "SORTED(" in text and "SCAN(" not in text, (case, text)
            got = oracle.execute(seg, count_spec(flt)).aggregations[0].count
            assert got == case["segment_count"], case
    finally:
        hseg.destroy()


def test_not_operator_plans_are_sorted_doc_ranges():
    seg = not_segment()
    hseg = host.HostSegment(seg, string_dicts=seg.string_dicts, load=False)
    try:
        ex = lambda f: host.explain_filter(hseg, "SELECT COUNT(*) FROM testTable WHERE " + f)
        assert ex("NOT FIRST_INT_COL = 5") == "NOT(SORTED(FIRST_INT_COL docs 5..5))"
        assert ex("NOT FIRST_INT_COL < 5") == "NOT(SORTED(FIRST_INT_COL docs 0..4))"
        assert ex("FIRST_INT_COL NOT BETWEEN 10 AND 20") == ex("NOT FIRST_INT_COL BETWEEN 10 AND 20") == "NOT(SORTED(FIRST_INT_COL docs 10..20))"
        assert ex("NOT (FIRST_INT_COL > 5 AND SECOND_INT_COL < 1009)") == "NOT(AND(SORTED(FIRST_INT_COL docs 6..1023), SORTED(SECOND_INT_COL docs 0..8)))"
        assert ex("NOT (FIRST_INT_COL < 5 OR SECOND_INT_COL > 2000)") == "NOT(OR(SORTED(FIRST_INT_COL docs 0..4), SORTED(SECOND_INT_COL docs 1001..1023)))"
    finally:
        hseg.destroy()


# ---- raw FLOAT / DOUBLE precision: expected values from numpy primitive compares on the literal parsed in the column's precision ----------
FP_EDGE_PRECISION_SQL = [
    # (column, WHERE clause, numpy predicate over the column's values)
    ("f", "f > 0.1", lambda x: x > np.float32("0.1")),
    ("f", "f <= 0.3", lambda x: x <= np.float32("0.3")),
    ("f", "f = 0.7", lambda x: x == np.float32("0.7")),
    ("f", "f BETWEEN 0.1 AND 0.3", lambda x: (x >= np.float32("0.1")) & (x <= np.float32("0.3"))),
    ("f", "f > 0.0", lambda x: x > np.float32(0.0)),
    ("f", "f >= -0.0", lambda x: x >= np.float32(-0.0)),
    ("f", "f < -0.0", lambda x: x < np.float32(-0.0)),
    ("f", "f <= 0.0", lambda x: x <= np.float32(0.0)),
    ("f", "f = -0.0", lambda x: x == np.float32(-0.0)),
    ("f", "f <> 0.0", lambda x: x != np.float32(0.0)),
    ("f", "f < 'Infinity'", lambda x: x < np.float32(np.inf)),
    ("f", "f > '-Infinity' AND f < 'Infinity'", lambda x: (x > np.float32(-np.inf)) & (x < np.float32(np.inf))),
    ("f", "f = 'NaN'", lambda x: x == np.float32(np.nan)),
    ("f", "f <> 'NaN'", lambda x: x != np.float32(np.nan)),
    ("f", "NOT f > 0.1", lambda x: ~(x > np.float32("0.1"))),
    ("d", "d > 0.1", lambda x: x > np.float64("0.1")),
    ("d", "d BETWEEN 0.1 AND 0.3", lambda x: (x >= 0.1) & (x <= 0.3)),
    ("d", "d < 0.0", lambda x: x < 0.0),
    ("d", "d >= -0.0 AND d <= 0.0", lambda x: (x >= -0.0) & (x <= 0.0)),
    ("d", "d > 4.9E-324", lambda x: x > 5e-324),
    ("d", "d <> 'NaN'", lambda x: x != np.nan),
]
FP_EDGE_INVALID_SQL = ["f > 'Infinity'", "f < '-Infinity'", "d > 'Infinity'", "d < '-Infinity'", "f > 'NaN'", "d < 'NaN'"]


def fp_edge_values(n):
    """-0.0, 0.0, NaN of both signs, +-inf, the smallest subnormals and float32(0.1) / 0.3 / 0.7 next to their neighbours, spread over n docs."""
    f = np.float32
    inf = np.inf
    specials = [f(-0.0), f(0.0), f(np.nan), -f(np.nan), f(inf), f(-inf), np.nextafter(f(0), f(1)), -np.nextafter(f(0), f(1)), f(0.1), f(0.3), f(0.7)]
    for x in (f("0.1"), f("0.3"), f("0.7")):
        specials += [np.nextafter(x, f(inf)), np.nextafter(x, f(-inf))]
    fv = np.resize(np.array(specials, dtype=np.float32), n)
    rng = np.random.default_rng(n)
    fv[::7] = rng.uniform(-1, 1, fv[::7].shape[0]).astype(np.float32)
    d = [-0.0, 0.0, np.nan, -np.nan, inf, -inf, 5e-324, -5e-324, 0.1, 0.3, np.nextafter(0.1, inf), np.nextafter(0.1, -inf),
         float(f("0.1")), float(np.nextafter(f("0.1"), f(inf))), 1e-10]
    dv = np.resize(np.array(d, dtype=np.float64), n)
    dv[::5] = rng.uniform(-1, 1, dv[::5].shape[0])
    return fv, dv


def fp_edge_segment(n):
    fv, dv = fp_edge_values(n)
    return S.SegmentData("fpedge", n, [S.Column.raw_typed("f", fv), S.Column.raw_typed("d", dv)]), fv, dv


def test_fp_precision_sql_on_the_oracle():
    seg, fv, dv = fp_edge_segment(3001)
    hseg = host.HostSegment(seg, load=False)
    try:
        for col, where, pred in FP_EDGE_PRECISION_SQL:
            text, planned = plan_of(seg, hseg, "SELECT COUNT(*) FROM t WHERE " + where)
            with np.errstate(invalid="ignore"):
                want = int(pred(fv if col == "f" else dv).sum())
            assert oracle.execute(seg, count_spec(planned)).aggregations[0].count == want, (where, text)
        for where in FP_EDGE_INVALID_SQL:
            with pytest.raises(host.HostError, match="Invalid range") as ei:
                host.explain_filter(hseg, "SELECT COUNT(*) FROM t WHERE " + where)
            assert ei.value.status == 1
        # a FLOAT literal is rounded once, to float; a DOUBLE literal stays double: the bounds differ
        f_text = host.explain_filter(hseg, "SELECT COUNT(*) FROM t WHERE f > 0.1")
        d_text = host.explain_filter(hseg, "SELECT COUNT(*) FROM t WHERE d > 0.1")
        assert f_text == "SCAN(f raw %d..%d)" % (Q.f64_bits(np.nextafter(np.float32("0.1"), np.float32(np.inf))), Q.f64_bits(np.inf))
        assert d_text == "SCAN(d raw %d..%d)" % (Q.f64_bits(np.nextafter(0.1, np.inf)), Q.f64_bits(np.inf))
    finally:
        hseg.destroy()
