"""CPU tests of PERCENTILE / DISTINCTCOUNT on raw columns: the C header and its Python mirror agree on the additions; the numpy model of
tests/raw_value_cases.py against hand-written lists; the order image's round trip at the edge values; the host mirror's raw-derived
intermediate results (ValueCounts::fromDeviceValues with its LONG-to-double run merge, ValueSet::fromDeviceValues) and the reference's
goldens through the host-only combines fed with them; and the engine's accept / decline decisions as its planners state them."""
import os
import re

import numpy as np
import pytest

import distinct_cases as D
import helpers as H
import percentile_cases as P
import raw_value_cases as R
from pinot_amd import _abi
from pinot_amd import host
from pinot_amd import query as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = np.iinfo(np.int64)


def test_the_header_and_its_mirror_agree_on_the_additions():
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+5\b", header) and _abi.PG_ABI_VERSION == 5
    assert re.search(r"\bPG_KERNEL_SCAN_COLLECT\s*=\s*18\b", header) and _abi.KERNEL_NAMES[18] == "scan_collect_kernel"
    assert re.search(r"\bPG_KERNEL_GROUP_COLLECT\s*=\s*19\b", header) and _abi.KERNEL_NAMES[19] == "group_collect_kernel"
    assert re.search(r"#define\s+PG_COLLECT_MAX_BYTES\s+\(1ull << 30\)", header) and _abi.PG_COLLECT_MAX_BYTES == 1 << 30
    assert "pg_result_value_counts" in header and any(name == "pg_result_value_counts" for name, _, _ in _abi.ABI_SYMBOLS)
    assert "pg_result_value_counts: no struct layout changed, one function added" in header


# ---- the model against hand-written lists ----
class FakeSegment:
    def __init__(self, values):
        self.raw_values = {0: values}
        self.num_docs = len(values)


def test_the_model_against_hand_written_lists():
    bits, counts = R.runs_of(np.array([3, -1, 3, 7, -1, 3], dtype=np.int32))
    assert bits.tolist() == [-1, 3, 7] and counts.tolist() == [2, 3, 1] and bits.dtype == np.int64 and counts.dtype == np.uint32
    bits, counts = R.runs_of(np.array([I64.max, I64.min, 0, I64.min], dtype=np.int64))
    assert bits.tolist() == [I64.min, 0, I64.max] and counts.tolist() == [2, 1, 1]
    # Double.compare's order: -inf < -1.5 < -0.0 < 0.0 < 1.5 < inf < NaN; every NaN is the one canonical NaN
    nan2 = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]
    bits, counts = R.runs_of(np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, nan2, -1.5, 0.0], dtype=np.float64))
    want = np.array([-np.inf, -1.5, -0.0, 0.0, 1.5, np.inf, np.nan], dtype=np.float64)
    assert np.array_equal(bits, want.view(np.int64)) and counts.tolist() == [1, 1, 1, 2, 1, 1, 2]
    # FLOAT is widened exactly: the bits are the double's
    bits, counts = R.runs_of(np.array([0.1, 0.1, -2.5], dtype=np.float32))
    assert np.array_equal(bits.view(np.float64), np.array([-2.5, float(np.float32(0.1))])) and counts.tolist() == [1, 2]
    # through model(): the filter's docs only, one entry per aggregation; an empty match is an empty list
    seg = FakeSegment(np.array([5, 5, 9, 1, 9, 9], dtype=np.int64))
    spec = Q.QuerySpec([(Q.PERCENTILE, 0), (Q.COUNT, -1), (Q.DISTINCTCOUNT, 0)])
    lists = R.model(seg, spec, match=np.array([1, 0, 1, 0, 1, 1], dtype=bool))
    assert sorted(lists) == [0, 2] and lists[0][0].tolist() == [5, 9] and lists[0][1].tolist() == [1, 3]
    assert R.model(seg, spec, match=np.zeros(6, dtype=bool))[2][0].shape == (0,)


EDGE_LONGS = np.array([I64.min, I64.min + 1, -(1 << 53) - 1, -1, 0, 1, (1 << 53), (1 << 53) + 1, I64.max - 1, I64.max], dtype=np.int64)
EDGE_DOUBLES = np.array([-np.inf, -np.finfo(np.float64).max, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.finfo(np.float64).max, np.inf, np.nan], dtype=np.float64)


def test_the_order_image_round_trips_and_keeps_the_order_at_the_edges():
    images = R.order_image(EDGE_LONGS)
    assert images.dtype == np.uint64 and (np.diff(images.astype(object)) > 0).all()
    assert np.array_equal(R.value_bits_of_image(images, False), EDGE_LONGS)
    images = R.order_image(np.array([np.iinfo(np.int32).min, -1, 0, np.iinfo(np.int32).max], dtype=np.int32))
    assert (np.diff(images.astype(object)) > 0).all() and R.value_bits_of_image(images, False).tolist() == [-(1 << 31), -1, 0, (1 << 31) - 1]
    images = R.order_image(EDGE_DOUBLES)
    assert (np.diff(images.astype(object)) > 0).all()                      # -0.0 below 0.0, NaN above +inf
    assert np.array_equal(R.value_bits_of_image(images, True), EDGE_DOUBLES.view(np.int64))
    # every NaN payload is one image; float32 edges are their widened doubles'
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)
    assert len(set(R.order_image(nans).tolist())) == 1
    f32 = np.array([-np.inf, -1.5, -0.0, 0.0, np.finfo(np.float32).tiny, np.inf], dtype=np.float32)
    assert np.array_equal(R.order_image(f32), R.order_image(f32.astype(np.float64)))
    # the device's functions are the ones the rank image was built with: moved, not changed
    header = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_order_image.h")).read()
    assert "if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) b = 0x7FF8000000000000ull;" in header and "return (b >> 63) ? ~b : (b | (1ull << 63));" in header
    unit = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_unit_rank_image.hip")).read()
    assert '#include "pg_order_image.h"' in unit and "order_image_of_double_bits(unsigned long long b) {" not in unit


# ---- the host mirror: what segments merge ----
def test_two_longs_that_share_a_double_become_one_run_and_stay_two_set_elements():
    a, b = 2 ** 53, 2 ** 53 + 1
    assert a != b and float(a) == float(b)
    bits, counts = R.runs_of(np.array([b, a, 5, a, b, b], dtype=np.int64))
    assert bits.tolist() == [5, a, b] and counts.tolist() == [1, 2, 3]
    values, n = host.value_counts_from_device(_abi.PG_TYPE_LONG, bits, counts)
    assert values.tolist() == [5.0, float(a)] and n.tolist() == [1, 5]
    assert host.value_set_from_device(_abi.PG_TYPE_LONG, bits).tolist() == [5, a, b]
    # INT: exact, nothing merges
    values, n = host.value_counts_from_device(_abi.PG_TYPE_INT, [-7, 0, 3], [2, 1, 4])
    assert values.tolist() == [-7.0, 0.0, 3.0] and n.tolist() == [2, 1, 4]
    # nothing matched
    values, n = host.value_counts_from_device(_abi.PG_TYPE_DOUBLE, [], [])
    assert values.shape == (0,) and n.shape == (0,) and host.value_set_from_device(_abi.PG_TYPE_FLOAT, []).shape == (0,)


def test_floating_runs_keep_their_values_and_the_set_ascends_as_images():
    bits, counts = R.runs_of(EDGE_DOUBLES)
    values, n = host.value_counts_from_device(_abi.PG_TYPE_DOUBLE, bits, counts)
    assert np.array_equal(values.view(np.int64), EDGE_DOUBLES.view(np.int64)) and (n == 1).all()          # -0.0 and 0.0 are two runs, NaN the last
    images = host.value_set_from_device(_abi.PG_TYPE_DOUBLE, bits)
    assert sorted(images.tolist()) == images.tolist() and sorted(images.tolist()) == sorted(EDGE_DOUBLES.view(np.int64).tolist())


def test_a_nan_in_two_segments_lists_merges_into_one_last_run():
    """A raw DOUBLE column can hold NaN: in the run-wise merge it sorts last (Double.compare) and equals itself."""
    nan_bits = np.array([0.5, np.nan], dtype=np.float64).view(np.int64)
    one = percentile_cell(_abi.PG_TYPE_DOUBLE, (nan_bits, np.array([1, 2], dtype=np.uint32)))
    other = percentile_cell(_abi.PG_TYPE_DOUBLE, (np.array([0.25, 0.5, np.nan]).view(np.int64), np.array([4, 1, 3], dtype=np.uint32)))
    out = host.combine_counts("SELECT PERCENTILE50(m), PERCENTILE100(m) FROM t", [[((), [one, one])], [((), [other, other])]])
    assert out["combined"]["intermediate"][0]["counts"] == [4, 2, 5] and out["combined"]["intermediate"][0]["values"][:2] == [0.25, 0.5]
    assert out["combined"]["final"][0] == 0.5 and out["combined"]["final"][1] == "NaN"


def percentile_cell(stored_type, pairs):
    values, counts = host.value_counts_from_device(stored_type, pairs[0], pairs[1])
    return (int(counts.sum()), 0.0, 0.0, 0.0, False, (values, counts))


def test_merge_and_final_result_of_raw_derived_lists_equal_a_brute_force_sort():
    rng = np.random.default_rng(8)
    ps = [0, 50, 99, 99.9, 100]
    sql = "SELECT %s FROM t" % ", ".join(("PERCENTILE%d(m)" % p if float(p).is_integer() else "PERCENTILE(m, %r)" % p) for p in ps)
    for dtype, stored in ((np.int32, _abi.PG_TYPE_INT), (np.int64, _abi.PG_TYPE_LONG), (np.float32, _abi.PG_TYPE_FLOAT), (np.float64, _abi.PG_TYPE_DOUBLE)):
        values = (rng.integers(-50, 50, 1000) * (3 if np.issubdtype(dtype, np.integer) else 0.75)).astype(dtype)
        parts = [values[:200], values[200:200], values[200:]]
        out = host.combine_counts(sql, [[((), [percentile_cell(stored, R.runs_of(part))] * len(ps))] for part in parts])
        s = np.sort(values.astype(np.float64))
        want = [float(s[-1] if p == 100 else s[int(float(len(s)) * p / 100.0)]) for p in ps]
        assert out["combined"]["final"] == want, (dtype, out["combined"]["final"], want)


# ---- the reference's goldens from the fixture's RAW values through the host-only combines ----
@pytest.fixture(scope="module")
def golden():
    seg = H.golden_segment()          # (the filter and the keys are the dictionary columns'; the values are read as a raw column's would be)
    d = H.load_golden_columns()
    ci = seg.column_index
    seg.raw_values = {ci("column1"): np.asarray(d["column1"], dtype=np.int32), ci("column3"): np.asarray(d["column3"], dtype=np.int32)}
    models = {}
    for shape, (filtered, grouped) in P.GOLDEN_SHAPES.items():
        spec = P.golden_spec(seg, filtered, grouped)
        models[shape] = R.model(seg, spec)
    return seg, models


@pytest.mark.parametrize("p", [50, 90, 95, 99])
@pytest.mark.parametrize("shape", ["plain", "filter", "group", "filter+group"])
def test_the_sixteen_percentile_goldens_from_raw_derived_lists(golden, shape, p):
    seg, models = golden
    lists = models[shape]
    sql = "SELECT PERCENTILE%d(column1) AS v1, PERCENTILE%d(column3) AS v2 FROM testTable" % (p, p)
    cell = lambda pairs: percentile_cell(_abi.PG_TYPE_INT, pairs)
    if P.GOLDEN_SHAPES[shape][1]:
        c9 = seg.columns[seg.column_index("column9")]
        block = [((int(c9.value_of(gid)),), [cell(l[0]), cell(l[1])]) for gid, l in sorted(lists.items())]
        out = host.combine_counts(sql + " GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1", [block] * 4, [host.KEY_INT])
        assert out["resultTable"]["rows"] == [list(P.GOLDEN_VALUES[(p, shape)])]
    else:
        block = [((), [cell(lists[0]), cell(lists[1])])]
        assert sum(c[0] for c in block[0][1]) == 2 * P.GOLDEN_STATS[shape][0]
        out = host.combine_counts(sql, [block] * 4)
        assert out["combined"]["final"] == list(P.GOLDEN_VALUES[(p, shape)])


@pytest.mark.parametrize("shape", ["group", "filter+group"])
def test_the_grouped_distinctcount_goldens_from_raw_derived_sets(golden, shape):
    seg, models = golden
    lists = models[shape]
    c9 = seg.columns[seg.column_index("column9")]
    cell = lambda pairs: (0, 0.0, 0.0, 0.0, False, host.value_set_from_device(_abi.PG_TYPE_INT, pairs[0]).tolist())
    block = [((int(c9.value_of(gid)),), [cell(l[0]), cell(l[1])]) for gid, l in sorted(lists.items())]
    sql = "SELECT DISTINCTCOUNT(column1) AS v1, DISTINCTCOUNT(column3) AS v2 FROM testTable GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1"
    out = host.group_by_combine(sql, [block] * 4, [host.KEY_INT])
    row = D.GOLDEN_ROWS[shape]
    assert out["reduced"] == [[D.GOLDEN_GROUP_KEY, row["v1"], row["v2"]]]


def test_the_plain_distinctcount_goldens_are_the_models_run_counts(golden):
    _, models = golden
    for shape in ("plain", "filter"):
        row = D.GOLDEN_ROWS[shape]
        assert (len(models[shape][0][0]), len(models[shape][1][0])) == (row["v1"], row["v2"])


# ---- what the planners accept and decline, as they state it ----
def test_the_planners_route_raw_columns_to_the_collect_pass_and_name_every_decline():
    engine = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_engine.hip")).read()
    for function, begin, end in (("PERCENTILE", "static pg_status plan_percentile", "static int64_t append_count_row"),
                                 ("DISTINCTCOUNT", "static pg_status plan_distinct", "static void distinct_agg_value")):
        plan = engine[engine.index(begin):engine.index(end)]
        # the filter walk and the GROUP BY key space are planned by helpers the two planners share: their text counts as the planner's
        assert "plan_pass_filter(seg, q, " in plan and "plan_pass_keys(seg, q, " in plan
        plan += engine[engine.index("static pg_status plan_pass_filter"):engine.index("static pg_status split_pass_query")]
        assert "raw (no-dictionary) column" not in plan                                        # the old decline is gone
        assert "plan_collect_column(col, \"%s\")" % function in plan and "plan_collect_bytes(seg, \"%s\", raw_cols.size(), ng > 0)" % function in plan
        assert "kQueryCollectPass" in plan
        for message in ("on raw column %s and dictionary column %s in one query", "which carries a null value vector, under null handling",
                        "beside a range predicate on raw LONG / FLOAT / DOUBLE column", "which is not keyed by offset", "above numGroupsLimit"):
            assert message in plan, (function, message)
    assert "PERCENTILE beside DISTINCTCOUNT in one query" in engine
    # opt-in: off unless PINOT_GPU_COLLECT=1, and then the decline names the switch
    assert "bool collect = false;" in engine and 'getenv("PINOT_GPU_COLLECT"); g_engine.collect = cv != nullptr && cv[0] == \'1\';' in engine
    column = engine[engine.index("static pg_status plan_collect_column"):engine.index("// The pass's lists -> the result's.")]
    assert "if (!g_engine.collect)" in column and "the collect pass is off (PINOT_GPU_COLLECT=1 turns it on)" in column
    bound = engine[engine.index("static pg_status plan_collect_bytes"):engine.index("static pg_status plan_collect_column")]
    assert "16ull * (unsigned long long)columns + (grouped ? 8ull : 0ull)" in bound and "seg->num_docs" in bound
    assert "PG_COLLECT_MAX_BYTES" in bound and "g_engine.group_table_bytes" in bound
    # a caller cannot set the pass's flag: every bit above the public ones is refused at the entry points
    assert "constexpr int32_t kQueryCollectPass = 1 << 26;" in engine and "(q->flags & ~kQueryPublicFlags) != 0" in engine
