"""RangeQueriesTest / NotOperatorQueriesTest on the device: the goldens of tests/golden/range_queries_kats.json and not_operator_kats.json
through SQL verbatim (the C++ planner + HIP kernels), through the filter bitmap, through every kernel family that takes them, over scaled
replicas whose expected values come from the fixture formula and numpy (never from the oracle), in one batch, and the raw FLOAT / DOUBLE
compares at signed zeros, NaN, infinities and float32 neighbours."""
import json
import os

import numpy as np
import pytest

import helpers as H
from pinot_amd import _abi
from pinot_amd import host
from pinot_amd import query as Q
from test_oracle_range_not_queries import (FP_EDGE_INVALID_SQL, FP_EDGE_PRECISION_SQL, NOT_KATS, NOT_PERIOD, RANGE_KATS, RANGE_PERIOD,
                                           fp_edge_segment, like_dict_set, not_segment, plan_of, range_segment, range_values, selection_mask)

pytestmark = pytest.mark.gpu

NOT_SQL_CASES = [c for c in NOT_KATS["cases"] if c["group"] != "like"]
BROKER = NOT_KATS["broker_factor"]


@pytest.fixture(scope="module")
def plan_maker():
    import torch  # noqa: F401
    host.init_plan_maker(device=0, time_kernels=True)


def _count_of(block):
    return int(block["intermediate"][0])


@pytest.mark.parametrize("raw_int_dictionary", [False, True])
def test_range_count_goldens_through_sql(plan_maker, raw_int_dictionary):
    """testCountOverRangeFilter (and ...AfterReload with rawIntCol dictionary-encoded): the SQL verbatim, one segment and the broker's
    combination of four; for rawFloatCol / rawDoubleCol this is SQL reaching the raw FLOAT / DOUBLE leaves."""
    data = range_segment(raw_int_dictionary=raw_int_dictionary)
    segs = [host.HostSegment(data) for _ in range(4)]
    try:
        for case in RANGE_KATS["count_cases"]:
            one = host.execute_sql(segs[:1], case["sql"])
            assert _count_of(one["segments"][0]) == case["count"], case
            four = host.execute_sql(segs, case["sql"], max_execution_threads=4)
            assert [_count_of(b) for b in four["segments"]] == [case["count"]] * 4, case
            assert int(four["combined"]["final"][0]) == 4 * case["count"], case
    finally:
        [s.destroy() for s in segs]


def test_not_operator_goldens_through_sql(plan_maker):
    """testRangePredicates / testCompositePredicates: per segment the golden, at the broker (four segments) BROKER x the golden."""
    data = not_segment()
    segs = [host.HostSegment(data, string_dicts=data.string_dicts) for _ in range(4)]
    try:
        for case in NOT_SQL_CASES:
            sql = NOT_KATS["query"].replace("<filter>", case["filter"])
            assert _count_of(host.execute_sql(segs[:1], sql)["segments"][0]) == case["segment_count"], case
            assert int(host.execute_sql(segs, sql, max_execution_threads=4)["combined"]["final"][0]) == BROKER * case["segment_count"], case
    finally:
        [s.destroy() for s in segs]


def _bits(words, n):
    return np.unpackbits(np.asarray(words, dtype="<u8").view(np.uint8), bitorder="little")[:n].astype(bool)


def test_range_selection_goldens_through_the_filter_bitmap(engine):
    data = range_segment()
    hseg = host.HostSegment(data, load=False)
    v = range_values(RANGE_PERIOD)
    try:
        with engine.open(data) as g:
            for case, count in zip(RANGE_KATS["selection_cases"], RANGE_KATS["count_cases"]):
                _, flt = plan_of(data, hseg, count["sql"])
                words, card = g.filter_bitmap(Q.QuerySpec([(Q.COUNT, -1)], filter=flt))
                assert np.array_equal(_bits(words, RANGE_PERIOD), selection_mask(v, case)), case
                assert card == count["count"], case
    finally:
        hseg.destroy()


def _golden_specs(data, hseg, which):
    """(label, spec, expected count) for every count golden of a fixture segment, lowered by the C++ planner (LIKE: by hand, see like_dict_set)."""
    out = []
    if which == "range":
        for case in RANGE_KATS["count_cases"]:
            _, flt = plan_of(data, hseg, case["sql"])
            shape = "eq" if " = " in case["sql"] else ("between" if case["inclusive"] else "gt_and_lt")
            encoding = "dict" if data.column(case["column"]).dictionary is not None else "raw"
            out.append(((case["column"], encoding, shape), Q.QuerySpec([(Q.COUNT, -1)], filter=flt), case["count"]))
    else:
        for case in NOT_KATS["cases"]:
            flt = like_dict_set(data, case) if case["group"] == "like" else plan_of(data, hseg, NOT_KATS["query"].replace("<filter>", case["filter"]))[1]
            out.append((("DOMAIN_NAMES", "dict set", "like") if case["group"] == "like" else ("FIRST_INT_COL / SECOND_INT_COL", "sorted", case["group"]), Q.QuerySpec([(Q.COUNT, -1)], filter=flt),
                        case["segment_count"]))
    return out


# the kernel families the goldens must reach (pg_execute's dominant kernel of COUNT(*) under the golden's filter)
FAMILY_SWITCHES = [{}, {"PINOT_GPU_SCAN_RAW": "0"}, {"PINOT_GPU_SCAN_SIMPLE": "0"}, {"PINOT_GPU_SET_LDS": "0"}, {"PINOT_GPU_FSM_EPISODES": "0"}]


def test_goldens_reach_every_kernel_family(engine):
    """Every count golden of both fixtures on the device, under the default routing and under each PINOT_GPU_* switch that sends the same
    query to another family; the families reached are recorded per (column encoding, query shape)."""
    fixtures = []
    for which, data in (("range", range_segment()), ("range", range_segment(raw_int_dictionary=True)), ("not", not_segment())):
        hseg = host.HostSegment(data, string_dicts=getattr(data, "string_dicts", None), load=False)
        fixtures.append((data, _golden_specs(data, hseg, which)))
        hseg.destroy()
    families = {}
    try:
        for env in FAMILY_SWITCHES:
            engine.reinit(**{k: env.get(k) for e in FAMILY_SWITCHES for k in e})
            for data, specs in fixtures:
                with engine.open(data) as g:
                    for label, spec, want in specs:
                        got = g.execute(spec)
                        assert got.aggregations[0].count == want, (env, label)
                        families.setdefault(got.dominant_kernel, set()).add((tuple(sorted(env)),) + label)
    finally:
        engine.reinit(**{k: None for env in FAMILY_SWITCHES for k in env})
    out = os.environ.get("PINOT_GPU_TEST_FAMILY_LOG")
    if out:
        with open(out, "w") as f:
            json.dump({k: sorted(map(list, v)) for k, v in families.items()}, f, indent=1)
    default = {label[1:]: k for k, labels in families.items() for label in labels if label[0] == ()}
    # the default routing: raw INT ranges in scan_raw_kernel, raw LONG / FLOAT / DOUBLE leaves in the general scan_agg_kernel, a one-leaf
    # dictionary range in scan_simple_kernel, the exclusive LIKE sets of the 4-bit DOMAIN_NAMES in scan_narrow_kernel, the sorted doc ranges
    # under NOT in scan_private_kernel
    assert default[("rawIntCol", "raw", "between")] == "scan_raw_kernel"
    for col in ("rawLongCol", "rawFloatCol", "rawDoubleCol"):
        for shape in ("between", "gt_and_lt", "eq"):
            assert default[(col, "raw", shape)] == "scan_agg_kernel", (col, shape)
    assert default[("dictionarizedIntCol", "dict", "between")] == "scan_simple_kernel"
    assert default[("DOMAIN_NAMES", "dict set", "like")] == "scan_narrow_kernel"
    assert default[("FIRST_INT_COL / SECOND_INT_COL", "sorted", "range")] == default[("FIRST_INT_COL / SECOND_INT_COL", "sorted", "composite")] == "scan_private_kernel"
    # PINOT_GPU_SCAN_RAW=0 / SCAN_SIMPLE=0 / SET_LDS=0 move the raw INT ranges, the dictionary ranges and the LIKE sets to scan_private_kernel
    moved = {(label[0], label[1:]) for label in families.get("scan_private_kernel", ())}
    assert (("PINOT_GPU_SCAN_RAW",), ("rawIntCol", "raw", "between")) in moved
    assert (("PINOT_GPU_SCAN_SIMPLE",), ("dictionarizedIntCol", "dict", "between")) in moved
    assert (("PINOT_GPU_SET_LDS",), ("DOMAIN_NAMES", "dict set", "like")) in moved


def _scaled_expectations(n, which):
    """Expected counts of a fixture repeated over n docs: (n // period) x the golden + a numpy count over the partial copy at the end."""
    if which == "range":
        v = range_values(n % RANGE_PERIOD)
        return [(n // RANGE_PERIOD) * c["count"] + int(selection_mask(v, c).sum()) for c in RANGE_KATS["count_cases"]]
    i = np.arange(n % NOT_PERIOD)
    first, second = i, 1000 + i
    names = NOT_KATS["domain_names"]
    dom = np.array([names[k % 16] for k in i], dtype=object)
    partial = {
        "NOT FIRST_INT_COL = 5": ~(first == 5), "NOT FIRST_INT_COL < 5": ~(first < 5), "NOT FIRST_INT_COL > 5": ~(first > 5),
        "FIRST_INT_COL NOT BETWEEN 10 AND 20": ~((first >= 10) & (first <= 20)), "NOT FIRST_INT_COL BETWEEN 10 AND 20": ~((first >= 10) & (first <= 20)),
        "NOT (FIRST_INT_COL > 5 AND SECOND_INT_COL < 1009)": ~((first > 5) & (second < 1009)),
        "NOT FIRST_INT_COL > 5 OR NOT SECOND_INT_COL < 1009": ~(first > 5) | ~(second < 1009),
        "NOT (FIRST_INT_COL < 5 OR SECOND_INT_COL > 2000)": ~((first < 5) | (second > 2000)),
        "NOT FIRST_INT_COL < 5 AND NOT SECOND_INT_COL > 2000": ~(first < 5) & ~(second > 2000)}
    out = []
    for c in NOT_KATS["cases"]:
        if c["group"] == "like":
            words = like_dict_set(not_segment(16), c).pred.set_words
            sorted_names = sorted(names)
            got = sum(1 for s in dom if not (int(words[sorted_names.index(s) >> 5]) >> (sorted_names.index(s) & 31)) & 1)
        else:
            got = int(partial[c["filter"]].sum())
        out.append((n // NOT_PERIOD) * c["segment_count"] + got)
    return out


def _scaled_not_segment(n):
    """The NotOperatorQueriesTest rows repeated every 1 024 docs (past 1 024 the INT columns are no longer sorted: dictionary scans)."""
    from pinot_amd import segment as S
    i = (np.arange(n) % NOT_PERIOD).astype(np.int32)
    names = NOT_KATS["domain_names"]
    sorted_names = sorted(names)
    ids = np.array([sorted_names.index(s) for s in names], dtype=np.int32)[i % 16]
    seg = S.SegmentData("notScaled", n, [S.Column.dict_encoded("FIRST_INT_COL", i), S.Column.dict_encoded("SECOND_INT_COL", 1000 + i),
                                         S.Column.from_dict_ids("DOMAIN_NAMES", np.arange(16, dtype=np.int32), ids)])
    seg.string_dicts = {"DOMAIN_NAMES": sorted_names}
    return seg


def _check_scaled(engine, n):
    rdata = range_segment(n, name="rangeScaled")
    v = range_values(n)
    lv, dv = v.astype(np.int64), v.astype(np.float64)
    hseg = host.HostSegment(rdata, load=False)
    specs = _golden_specs(rdata, hseg, "range")
    hseg.destroy()
    li, di = rdata.column_index("rawLongCol"), rdata.column_index("rawDoubleCol")
    with engine.open(rdata) as g:
        for (label, spec, _), want, case in zip(specs, _scaled_expectations(n, "range"), RANGE_KATS["count_cases"]):
            agg = Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, li), (Q.MIN, li), (Q.MAX, li), (Q.SUM, di), (Q.MIN, di), (Q.MAX, di)], filter=spec.filter)
            got = g.execute(agg).aggregations
            sel = selection_mask(v, case)
            assert got[0].count == want == int(sel.sum()), (n, label)
            assert got[1].sum_i64 == int(lv[sel].sum()), (n, label)
            assert abs(got[4].sum - float(dv[sel].sum())) <= H.FP_SUM_RTOL * max(abs(float(dv[sel].sum())), 1.0), (n, label)
            if want:
                assert (got[2].min, got[3].max) == (float(lv[sel].min()), float(lv[sel].max())), (n, label)
                assert (got[5].min, got[6].max) == (float(dv[sel].min()), float(dv[sel].max())), (n, label)
    if n > 20_000_000:
        return
    ndata = _scaled_not_segment(n)
    hseg = host.HostSegment(ndata, string_dicts=ndata.string_dicts, load=False)
    specs = _golden_specs(ndata, hseg, "not")
    hseg.destroy()
    with engine.open(ndata) as g:
        for (label, spec, _), want in zip(specs, _scaled_expectations(n, "not")):
            assert g.execute(spec).aggregations[0].count == want, (n, label)


@pytest.mark.parametrize("n", [1000, 1024, 2047, 2048, 2049])
def test_scaled_replicas_tile_tails(engine, n):
    _check_scaled(engine, n)


def test_scaled_replicas_many_tiles_per_wave(engine, monkeypatch):
    """300 017 docs on a grid sized for one compute unit (PINOT_GPU_TEST_CUS=1, read when a segment is opened): waves take several tiles."""
    monkeypatch.setenv("PINOT_GPU_TEST_CUS", "1")
    _check_scaled(engine, 300_017)


def test_scaled_replicas_full_grid(engine):
    _check_scaled(engine, 12_000_517)


def test_all_count_goldens_in_one_batch(engine):
    """Every count golden of both fixtures as items of one pg_execute_batch over 64 segment copies, the fixtures' encodings mixed so that items
    of different kinds (raw INT / LONG / FLOAT / DOUBLE, dictionary, sorted doc ranges, set leaves) share launches."""
    kinds = []
    for which, data in (("range", range_segment()), ("range", range_segment(raw_int_dictionary=True)), ("not", not_segment())):
        hseg = host.HostSegment(data, string_dicts=getattr(data, "string_dicts", None), load=False)
        kinds.append((data, _golden_specs(data, hseg, which)))
        hseg.destroy()
    items = [(data, label, spec, want) for data, specs in kinds for label, spec, want in specs]
    assert len(items) >= 64
    opened = {id(data): engine.open(data) for data, _ in kinds}
    try:
        for start in range(0, len(items), 64):
            chunk = items[start:start + 64]
            gsegs = [opened[id(d)] for d, _, _, _ in chunk]
            for (status, res), (d, label, spec, want), gs in zip(engine.execute_batch(gsegs, [it[2] for it in chunk]), chunk, gsegs):
                assert status == _abi.PG_OK, label
                assert res.aggregations[0].count == want, label
                single = gs.execute(spec)
                assert single.aggregations[0].count == want and res.stats == single.stats, label
    finally:
        [g.close() for g in opened.values()]


@pytest.mark.parametrize("n", [70_001])
def test_fp_edges_through_sql(plan_maker, n):
    """Raw FLOAT / DOUBLE columns seeded with -0.0, 0.0, NaN of both signs, +-inf, subnormals and float32(0.1) next to its neighbours, over
    many tiles: the precision SQL through the device against numpy primitive compares on the literal parsed in the column's precision."""
    data, fv, dv = fp_edge_segment(n)
    seg = host.HostSegment(data)
    try:
        for col, where, pred in FP_EDGE_PRECISION_SQL:
            with np.errstate(invalid="ignore"):
                want = int(pred(fv if col == "f" else dv).sum())
            assert _count_of(host.execute_sql([seg], "SELECT COUNT(*) FROM t WHERE " + where)["segments"][0]) == want, where
        for where in FP_EDGE_INVALID_SQL:
            with pytest.raises(host.HostError, match="Invalid range"):
                host.execute_sql([seg], "SELECT COUNT(*) FROM t WHERE " + where)
    finally:
        seg.destroy()
