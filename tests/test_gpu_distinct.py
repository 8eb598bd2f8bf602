"""DISTINCTCOUNT on dictionary columns on the device (PG_AGG_DISTINCTCOUNT, pg_result_distinct_dict_ids), through the C ABI.

Expected values: the reference's own numbers (InterSegmentAggregationSingleValueQueriesTest.testDistinctCount :235-258 over the committed
fixture) and the exact model of tests/distinct_cases.py (np.unique of the dictIds of the docs oracle.filter_bitmap matches); every other
function of a mixed query against the unchanged oracle.  Sets are compared element for element: there are no tolerances."""
import ctypes as C

import numpy as np
import pytest

import distinct_cases as D
import helpers as H
from oracle import oracle
from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S

pytestmark = pytest.mark.gpu

SCAN, GROUP = "scan_distinct_kernel", "group_distinct_kernel"
SWITCH = "PINOT_GPU_DISTINCT_LDS"
DC = Q.DISTINCTCOUNT


@pytest.fixture(scope="module")
def golden():
    seg = H.golden_segment()
    return seg, {}          # the segment, and the models of its queries (computed once, shared, never changed)


def golden_model(golden, filtered, grouped):
    seg, cache = golden
    if (filtered, grouped) not in cache:
        cache[(filtered, grouped)] = D.model(seg, D.golden_spec(seg, filtered, grouped))
    return cache[(filtered, grouped)]


def check_golden(got, golden, filtered, grouped, form="physical"):
    """The reference's statistics are those of ITS operator tree: H.golden_filter_physical (63064 entries in the filter).  The same predicates
    written as the logical tree, with or without postings, are other iterator trees over the same docs: their numEntriesScannedInFilter is
    what it is today for that filter -- the oracle's exact count -- and the other three statistics are the reference's."""
    seg, _ = golden
    spec = D.golden_spec(seg, filtered, grouped, form)
    row = D.GOLDEN_ROWS[("filter" if filtered else "") + ("+" if filtered and grouped else "") + ("group" if grouped else "") or "plain"]
    entries = row["stats"][1] if (form == "physical" or not filtered) else oracle.execute(seg, D.without_distinct(spec)).stats[1]
    want_stats = (row["stats"][0], entries, row["stats"][2], row["stats"][3])
    assert got.stats == want_stats and got.filter_entries_exact, (got.stats, want_stats, got.filter_entries_exact)
    D.assert_sets_equal(got, seg, spec, want=golden_model(golden, filtered, grouped))
    if grouped:
        top = got.groups[D.golden_group_id(seg)]
        assert (top[0].count, top[1].count) == (row["v1"], row["v2"])
        # ORDER BY v1 DESC, v2 DESC LIMIT 1 picks that group
        assert max(got.groups, key=lambda g: (got.groups[g][0].count, got.groups[g][1].count)) == D.golden_group_id(seg)
    else:
        assert (got.aggregations[0].count, got.aggregations[1].count) == (row["v1"], row["v2"])


# ---- 1. the reference's goldens through the C ABI ----
@pytest.mark.parametrize("grouped", [False, True])
def test_goldens_without_a_filter(engine, golden, grouped):
    seg, _ = golden
    with engine.open(seg) as g:
        got = g.execute(D.golden_spec(seg, False, grouped))
        check_golden(got, golden, False, grouped)
        if not grouped:
            assert got.dominant_kernel_ms == 0.0          # answered from the dictionaries: nothing was launched
        # a filter that matches everything is the same plan
        everything = Q.QuerySpec(D.golden_spec(seg, False, grouped).aggregations, filter=Q.leaf(Q.Pred.match_all()), group_by=D.golden_spec(seg, False, grouped).group_by)
        check_golden(g.execute(everything), golden, False, grouped)


@pytest.mark.parametrize("form", ["logical", "inverted", "physical"])
@pytest.mark.parametrize("grouped", [False, True])
def test_goldens_under_the_filter_in_its_three_forms(engine, golden, grouped, form):
    seg, _ = golden
    with engine.open(seg) as g:
        got = g.execute(D.golden_spec(seg, True, grouped, form))
        check_golden(got, golden, True, grouped, form)


def test_goldens_through_execute_batch_and_in_the_hbm_tier(engine, golden):
    seg, _ = golden
    shapes = [(False, False), (True, False), (True, True)]
    with engine.open(seg) as g:
        for (f, grp), (status, got) in zip(shapes, engine.execute_batch([g] * 3, [D.golden_spec(seg, f, grp, "physical") for f, grp in shapes])):
            assert status == _abi.PG_OK
            check_golden(got, golden, f, grp)
    engine.reinit(**{SWITCH: "0"})
    try:
        with engine.open(seg) as g:
            for f, grp in shapes + [(False, True)]:
                check_golden(g.execute(D.golden_spec(seg, f, grp, "physical")), golden, f, grp)
    finally:
        engine.reinit(**{SWITCH: None})


# ---- 2. the reference's goldens through SQL: the host mirror over four copies of the segment ----
SQL_QUERY = "SELECT DISTINCTCOUNT(column1) AS v1, DISTINCTCOUNT(column3) AS v2 FROM testTable"
SQL_FILTER = (" WHERE column1 > 100000000 AND column3 BETWEEN 20000000 AND 1000000000 AND column5 = 'gFuH'"
              " AND (column6 < 500000000 OR column11 NOT IN ('t', 'P')) AND daysSinceEpoch = 126164076")
SQL_GROUP_BY = " GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1"
# testDistinctCount :235-258: (query, numDocsScanned, numEntriesScannedInFilter, numEntriesScannedPostFilter, numTotalDocs, the row)
SQL_GOLDENS = [(SQL_QUERY, 120000, 0, 0, 120000, [6582, 21910]),
               (SQL_QUERY + SQL_FILTER, 24516, 252256, 49032, 120000, [1872, 4556]),
               (SQL_QUERY + SQL_GROUP_BY, 120000, 0, 360000, 120000, [3495, 11961]),
               (SQL_QUERY + SQL_FILTER + SQL_GROUP_BY, 24516, 252256, 73548, 120000, [1272, 3289])]


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
        assert out["resultTable"]["rows"] == [row], sql                  # the SELECT list shows the two INT finals of the LIMIT 1 row
        assert all(isinstance(x, int) for x in out["resultTable"]["rows"][0])
    else:
        assert out["combined"]["final"] == row, sql                      # four copies of the segment: the union is the segment's set
        assert [len(v["values"]) for v in out["combined"]["intermediate"]] == row
        assert [len(v["values"]) for v in out["segments"][0]["intermediate"]] == row


def test_datatable_bytes_of_a_value_set_are_declined(golden_host_segments):
    from pinot_amd import host
    with pytest.raises(host.HostError) as e:
        host.execute_sql_datatable(golden_host_segments[:1], SQL_QUERY + SQL_FILTER)
    assert e.value.status == 2 and "DISTINCTCOUNT" in str(e.value)
    # FILTER (WHERE ...) beside it keeps the CPU plan
    with pytest.raises(host.HostError) as e:
        host.execute_sql(golden_host_segments[:1], "SELECT DISTINCTCOUNT(column1), COUNT(*) FILTER (WHERE column1 > 100000000) FROM testTable")
    assert e.value.status == 2


# ---- 3. edges of the bitset ----
EDGE_CARDS = [1, 31, 32, 33, 4097, 100000]


@pytest.fixture(scope="module")
def edge_segment():
    return D.synthetic_segment(S, "distinct_edges", 100003, EDGE_CARDS + [1000])


def raw_words(g, spec, aggregation, row=-1):
    """(status, words) straight from the accessor, before the result is freed."""
    res = _abi.pg_result()
    _abi.check(g.lib, g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res)))
    try:
        words, n = C.POINTER(C.c_uint32)(), C.c_int32(-1)
        status = g.lib.pg_result_distinct_dict_ids(C.byref(res), aggregation, row, C.byref(words), C.byref(n))
        return status, (np.ctypeslib.as_array(words, shape=(n.value,)).copy() if status == _abi.PG_OK and n.value else np.zeros(0, np.uint32)), n.value
    finally:
        g.lib.pg_result_free(C.byref(res))


@pytest.mark.parametrize("lds", ["1", "0"])
def test_bitset_edges_in_both_tiers(engine, edge_segment, lds):
    seg = edge_segment
    flt = Q.leaf(Q.Pred.dict_range(len(EDGE_CARDS), 0, 700))          # 70 % of the docs
    engine.reinit(**{SWITCH: lds})
    try:
        with engine.open(seg) as g:
            for first in (0, 3):                                       # at most four columns per query
                cols = list(range(first, min(first + 3, len(EDGE_CARDS))))
                spec = Q.QuerySpec([(DC, c) for c in cols], filter=flt)
                got = g.execute(spec)
                assert got.dominant_kernel == SCAN
                D.assert_sets_equal(got, seg, spec)
                assert got.stats == (int(D.matching_docs(seg, spec).sum()), seg.num_docs, got.stats[0] * len(cols), seg.num_docs)
                for a, c in enumerate(cols):
                    card = EDGE_CARDS[c]
                    status, words, n = raw_words(g, spec, a)
                    assert status == _abi.PG_OK and n == (card + 31) // 32
                    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
                    assert not bits[card:].any(), "bits at and above the cardinality must be zero"
            # without a filter the docs are still scanned when a doc set says so; here: the last dictId is present in every set
            spec = Q.QuerySpec([(DC, c) for c in (0, 4, 5)], filter=Q.leaf(Q.Pred.dict_range(len(EDGE_CARDS), 0, 999)))
            got = g.execute(spec)
            for a, c in enumerate((0, 4, 5)):
                assert got.aggregations[a].dict_ids[-1] == EDGE_CARDS[c] - 1
            D.assert_sets_equal(got, seg, spec)
    finally:
        engine.reinit(**{SWITCH: None})


@pytest.mark.parametrize("num_docs", [31, 2049])
@pytest.mark.parametrize("lds", ["1", "0"])
def test_tiny_segments(engine, num_docs, lds):
    seg = D.synthetic_segment(S, "distinct_tiny_%d" % num_docs, num_docs, [33, 5, 4097])
    engine.reinit(**{SWITCH: lds})
    try:
        with engine.open(seg) as g:
            for flt in (Q.leaf(Q.Pred.dict_range(1, 1, 4)), Q.not_(Q.leaf(Q.Pred.dict_range(1, 0, 1)))):
                spec = Q.QuerySpec([(DC, 0), (DC, 2), (Q.COUNT, -1)], filter=flt)
                got = g.execute(spec)
                D.assert_sets_equal(got, seg, spec)
                assert got.aggregations[2].count == int(D.matching_docs(seg, spec).sum()) == got.stats[0]
    finally:
        engine.reinit(**{SWITCH: None})


# ---- 4. data shapes ----
@pytest.fixture(scope="module")
def shapes_segment():
    n = 100003
    rng = np.random.default_rng(21)
    same = np.full(n, 77, dtype=np.int32)
    cols = [S.Column.from_dict_ids("same", np.arange(5000, dtype=np.int32), same),
            S.Column.from_dict_ids("wide", np.arange(60000, dtype=np.int32) * 2, rng.integers(0, 60000, n).astype(np.int32)),
            S.Column.from_dict_ids("f", np.arange(1000, dtype=np.int32), rng.integers(0, 1000, n).astype(np.int32)),
            S.Column.from_dict_ids("x", np.arange(50, dtype=np.int32), rng.integers(0, 50, n).astype(np.int32), with_inverted=True),
            S.Column.from_dict_ids("y", np.arange(40, dtype=np.int32), rng.integers(0, 40, n).astype(np.int32), with_inverted=True)]
    return S.SegmentData("distinct_shapes", n, cols)


@pytest.mark.parametrize("lds", ["1", "0"])
def test_data_shapes(engine, shapes_segment, lds):
    seg = shapes_segment
    n = seg.num_docs
    engine.reinit(**{SWITCH: lds})
    try:
        with engine.open(seg) as g:
            # every doc the same dictId: all lanes hit one word
            spec = Q.QuerySpec([(DC, 0)], filter=Q.leaf(Q.Pred.dict_range(2, 0, 900)))
            got = g.execute(spec)
            assert list(got.aggregations[0].dict_ids) == [77] and got.aggregations[0].count == 1
            # a filter that matches nothing: count 0, words all zero, a set still returned
            spec = Q.QuerySpec([(DC, 1), (Q.COUNT, -1)], filter=Q.and_(Q.leaf(Q.Pred.dict_range(2, 0, 10)), Q.leaf(Q.Pred.dict_range(2, 500, 510))))
            got = g.execute(spec)
            assert got.aggregations[0].count == 0 and got.aggregations[0].dict_ids is not None and len(got.aggregations[0].dict_ids) == 0 and got.aggregations[1].count == 0
            status, words, nw = raw_words(g, spec, 0)
            assert status == _abi.PG_OK and nw == (60000 + 31) // 32 and not words.any()
            # about 1 doc in 1000
            spec = Q.QuerySpec([(DC, 1), (DC, 0)], filter=Q.leaf(Q.Pred.dict_range(2, 123, 124)))
            got = g.execute(spec)
            D.assert_sets_equal(got, seg, spec)
            assert 40 < got.stats[0] < 200
            # an index-led filter: the tile list
            spec = Q.QuerySpec([(DC, 1)], filter=Q.and_(Q.leaf(Q.Pred.dict_range(3, 3, 4, inverted=True)), Q.leaf(Q.Pred.dict_range(4, 5, 6, inverted=True)),
                                                        Q.leaf(Q.Pred.dict_range(2, 0, 500))))
            got = g.execute(spec)
            D.assert_sets_equal(got, seg, spec)
            want = oracle.execute(seg, D.without_distinct(spec))
            assert got.stats[:2] == want.stats[:2] and got.stats[2] == got.stats[0] and got.filter_entries_exact
            # a doc set alone, holding every doc: scanned, never answered from the dictionary
            dsid = g.create_doc_set(words=np.packbits(np.concatenate([np.ones(n, bool), np.zeros((-n) % 64, bool)]), bitorder="little").view(np.uint64))
            spec = Q.QuerySpec([(DC, 1)], filter=Q.leaf(Q.Pred.doc_set(dsid)))
            got = g.execute(spec)
            assert got.stats == (n, 0, n, n) and got.dominant_kernel == SCAN
            everything = Q.QuerySpec([(DC, 1)])
            assert np.array_equal(got.aggregations[0].dict_ids, D.model(seg, everything)[0])
            g.release_doc_set(dsid)
    finally:
        engine.reinit(**{SWITCH: None})


# ---- 5. the HBM tier by size ----
def test_a_dictionary_beyond_the_lds_tier(engine):
    n, card = 300007, 1300000
    rng = np.random.default_rng(8)
    ids = rng.integers(0, card, n).astype(np.int32)
    ids[5] = card - 1
    seg = S.SegmentData("distinct_big", n, [S.Column.from_dict_ids("big", np.arange(card, dtype=np.int32), ids),
                                            S.Column.from_dict_ids("f", np.arange(100, dtype=np.int32), rng.integers(0, 100, n).astype(np.int32))])
    assert seg.columns[0].bits == 21
    with engine.open(seg) as g:
        spec = Q.QuerySpec([(DC, 0)], filter=Q.leaf(Q.Pred.dict_range(1, 0, 60)))
        got = g.execute(spec)
        assert got.dominant_kernel == SCAN
        D.assert_sets_equal(got, seg, spec)


# ---- 5b. the tier boundary and the set area beside the bitsets: both sides of every edge of scan_grid's arithmetic (include/pinot_gpu.h
# PG_DISTINCT_LDS_MAX_DICT_IDS = B, tied to kLdsBudget by a static_assert in pg_engine.hip).  bitsets (whole words, rounded up to 16 bytes) + the
# staged set area (2048 words = 65536 bits, when the filter has a dictId-set leaf and PINOT_GPU_SET_LDS is on) <= kLdsBudget:
#   B - 65536      the set is staged behind the bitset and the two add up to the budget exactly;
#   B - 65536 + 1  the set no longer fits beside the bitset: it stays in memory, the bitset stays in LDS;
#   B              the bitset alone fits exactly;      B + 1  the HBM tier.
# Which branch ran is not visible from outside (one kernel id): the test holds the answer on both sides of every edge, with the HIGHEST dictId
# of the column among the matching docs -- an area that overlaps the last words of the bitset shows there and nowhere else.
EDGE_SET_BITS = 65536
EDGE_SET_CARDS = [13, 65536, 65537]          # an ordinary staged set; the set fills the area (the area's own fit edge); 17 bits: never staged


@pytest.fixture(scope="module")
def tier_edge_segment():
    b, n = _abi.PG_DISTINCT_LDS_MAX_DICT_IDS, 100003
    rng = np.random.default_rng(43)
    # columns 0-3: the DISTINCTCOUNT columns; 4-6: the set-leaf columns (5, of exactly 65536, is also the second column of the two-column case)
    cards = [b - EDGE_SET_BITS, b - EDGE_SET_BITS + 1, b, b + 1] + EDGE_SET_CARDS
    ids = [rng.integers(0, card, n).astype(np.int32) for card in cards]
    members = {c: (0, cards[c] // 2, cards[c] - 1) for c in (4, 5, 6)}
    # docs that carry the highest dictId of DISTINCTCOUNT column j (and of column 5 beside it) AND a member of every IN list: in the first tile, in a
    # middle tile and in the last, partial, tile
    for j in range(4):
        for t, doc in enumerate((7 + 64 * j, 2048 * 23 + 100 + j, n - 1 - j)):
            ids[j][doc] = cards[j] - 1
            for c in (4, 5, 6):
                ids[c][doc] = members[c][(j + t) % 3]
            if t == 0:
                ids[5][doc] = cards[5] - 1
    cols = [S.Column.from_dict_ids("c%d" % i, np.arange(card, dtype=np.int32), ids[i]) for i, card in enumerate(cards)]
    seg = S.SegmentData("distinct_tier_edges", n, cols)
    seg.members = members
    return seg


@pytest.mark.parametrize("set_lds", [None, "0"], ids=["sets-staged", "PINOT_GPU_SET_LDS=0"])
def test_the_tier_boundary_and_the_set_area_beside_the_bitsets(engine, tier_edge_segment, set_lds):
    seg = tier_edge_segment
    b = _abi.PG_DISTINCT_LDS_MAX_DICT_IDS
    assert [seg.columns[c].cardinality for c in range(4)] == [b - EDGE_SET_BITS, b - EDGE_SET_BITS + 1, b, b + 1]
    words = lambda c: (seg.columns[c].cardinality + 31) // 32
    assert (words(0) + words(5)) * 32 == b          # the two-column case: word counts that sum to exactly the budget
    leaf = lambda c: Q.leaf(Q.Pred.dict_set(c, list(seg.members[c]), seg.columns[c].cardinality))
    engine.reinit(PINOT_GPU_SET_LDS=set_lds)
    try:
        with engine.open(seg) as g:
            cases = [((c,), leaf(s)) for c in range(4) for s in (4, 5, 6)]
            # two columns that fill the budget: without a set leaf (an exact fit), and with one (the set stays in memory)
            cases += [((0, 5), Q.leaf(Q.Pred.dict_range(4, 0, 1))), ((5, 0), Q.not_(Q.leaf(Q.Pred.dict_range(4, 1, 13)))), ((0, 5), leaf(4)), ((0, 5), leaf(5))]
            for cols, flt in cases:
                spec = Q.QuerySpec([(DC, c) for c in cols] + [(Q.COUNT, -1)], filter=flt)
                where = "columns %r (%r dictIds)" % (cols, [seg.columns[c].cardinality for c in cols])
                got = g.execute(spec)
                assert got.dominant_kernel == SCAN, where
                D.assert_sets_equal(got, seg, spec, where=where)
                for a, c in enumerate(cols):
                    assert seg.columns[c].cardinality - 1 in got.aggregations[a].dict_ids, where
                assert got.aggregations[len(cols)].count == got.stats[0] > 0
                D.assert_other_functions_equal(got, seg, spec)
    finally:
        engine.reinit(PINOT_GPU_SET_LDS=None)


# ---- 6. mixes ----
def check_mix(g, seg, spec, key_values=None):
    got = g.execute(spec)
    D.assert_sets_equal(got, seg, spec, key_values=key_values)
    D.assert_other_functions_equal(got, seg, spec)
    return got


@pytest.fixture(scope="module")
def mix_segment():
    n = 100003
    rng = np.random.default_rng(31)
    ids = lambda card: rng.integers(0, card, n).astype(np.int32)
    long_vals = (rng.integers(0, 3000, n).astype(np.int64) - 1500) * (2 ** 33 + 7)
    dbl_vals = rng.integers(0, 2000, n).astype(np.float64) * 0.37 - 300.0
    key_raw = rng.integers(-40, 60, n).astype(np.int32)
    cols = [S.Column.from_dict_ids("a", np.arange(200, dtype=np.int32) * 2 - 100, ids(200)),           # 0: 8 bits
            S.Column.from_dict_ids("v", (np.arange(5000, dtype=np.int64) * 7 + 3).astype(np.int32), ids(5000)),   # 1: 13 bits
            S.Column.from_dict_ids("b", np.arange(13, dtype=np.int32) * 5, ids(13)),                   # 2: 4 bits
            S.Column.from_dict_ids("w2", np.arange(3, dtype=np.int32), ids(3)),                        # 3: 2 bits
            S.Column.from_dict_ids("w17", np.arange(100000, dtype=np.int32), ids(100000)),             # 4: 17 bits
            S.Column.dict_encoded_typed("dl", long_vals),                                              # 5: LONG-valued dictionary
            S.Column.dict_encoded_typed("dd", dbl_vals),                                               # 6: DOUBLE-valued dictionary
            S.Column.from_dict_ids("f", np.arange(1000, dtype=np.int32), ids(1000)),                   # 7
            S.Column.raw("kr", key_raw)]                                                               # 8: raw INT key
    seg = S.SegmentData("distinct_mix", n, cols)
    seg.key_raw = key_raw
    return seg


def test_mixes_with_other_functions(engine, mix_segment):
    seg = mix_segment
    f_lt = lambda t: Q.leaf(Q.Pred.dict_range(7, 0, t))
    with engine.open(seg) as g:
        check_mix(g, seg, Q.QuerySpec([(Q.COUNT, -1), (DC, 0), (Q.SUM, 1), (DC, 0), (Q.MAX, 2)], filter=f_lt(300)))
        check_mix(g, seg, Q.QuerySpec([(DC, 0), (Q.AVG, 1), (Q.MIN, 2)]))                                   # no filter, SUM in the mix: scanned
        got = check_mix(g, seg, Q.QuerySpec([(DC, 3), (DC, 0), (DC, 1), (DC, 4)], filter=Q.or_(f_lt(100), Q.leaf(Q.Pred.dict_set(2, [1, 5, 11], 13)))))
        assert got.dominant_kernel == SCAN
        check_mix(g, seg, Q.QuerySpec([(DC, 5), (DC, 6), (Q.COUNT, -1)], filter=f_lt(500)))
        check_mix(g, seg, Q.QuerySpec([(DC, 5), (Q.SUM, 5), (Q.MAX, 6), (DC, 6)], filter=f_lt(500)))
        # MIN / MAX / COUNT beside it and no filter: every function from the dictionaries
        spec = Q.QuerySpec([(Q.MIN, 1), (DC, 1), (Q.COUNT, -1), (Q.MAX, 6)])
        got = g.execute(spec)
        assert got.stats == (seg.num_docs, 0, 0, seg.num_docs)
        assert np.array_equal(got.aggregations[1].dict_ids, np.arange(5000)) and got.aggregations[1].count == 5000
        want = oracle.execute(seg, D.without_distinct(spec))
        H.assert_agg_equal(got.aggregations[0], want.aggregations[0], Q.MIN)
        H.assert_agg_equal(got.aggregations[3], want.aggregations[3], Q.MAX)


# ---- 7. GROUP BY beyond the goldens ----
def test_group_by_two_dictionary_keys_a_raw_key_and_emptied_groups(engine, mix_segment):
    seg = mix_segment
    f_lt = lambda t: Q.leaf(Q.Pred.dict_range(7, 0, t))
    with engine.open(seg) as g:
        got = check_mix(g, seg, Q.QuerySpec([(DC, 1), (Q.SUM, 1), (DC, 4)], filter=f_lt(400), group_by=[2, 0]))          # 13 x 200
        assert got.group_id_upper_bound == 2600
        # groups the filter empties are absent: only b in {1, 5} survives
        got = check_mix(g, seg, Q.QuerySpec([(DC, 1)], filter=Q.leaf(Q.Pred.dict_set(2, [1, 5], 13)), group_by=[2, 0]))
        assert len(got.groups) == 400 and all(gid % 13 in (1, 5) for gid in got.groups)
        assert got.dominant_kernel == GROUP
        # one raw INT key, keyed by offset
        base, is_offset, _ = g.group_key_info(8)
        assert is_offset == 1
        kv = {8: (seg.key_raw, base, int(seg.key_raw.max()) - int(seg.key_raw.min()) + 1)}
        check_mix(g, seg, Q.QuerySpec([(DC, 0), (Q.COUNT, -1)], filter=f_lt(250), group_by=[8]), key_values=kv)
    engine.reinit(**{SWITCH: "0"})
    try:
        with engine.open(seg) as g:
            check_mix(g, seg, Q.QuerySpec([(DC, 1), (Q.MAX, 2)], filter=f_lt(400), group_by=[2]))
    finally:
        engine.reinit(**{SWITCH: None})


# ---- 8. declines ----
def declined(g, spec, pattern):
    import re
    for call in (lambda: g.lib.pg_query_check(g.handle, C.byref(spec.c)), None):
        if call is not None:
            status = call()
        else:
            res = _abi.pg_result()
            status = g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res))
            g.lib.pg_result_free(C.byref(res))
        message = (g.lib.pg_last_error() or b"").decode()
        assert status == _abi.PG_ERR_UNSUPPORTED, (status, message)
        assert re.search(pattern, message), message


def test_declines_name_their_reason(engine, mix_segment):
    seg = mix_segment
    with engine.open(seg) as g:
        declined(g, Q.QuerySpec([(DC, 8)]), r"raw \(no-dictionary\) column kr")
        # a key space of kind 1 (beyond an int): 100000 x 5000 x 1000 x 200
        declined(g, Q.QuerySpec([(DC, 0)], group_by=[4, 1, 7, 0]), r"key space of kind 1")
        # group_id_upper_bound above numGroupsLimit
        declined(g, Q.QuerySpec([(DC, 0)], group_by=[1, 7]), r"above numGroupsLimit 100000")
        declined(g, Q.QuerySpec([(DC, 0)], group_by=[2, 0], num_groups_limit=2599), r"above numGroupsLimit 2599")
        g.execute(Q.QuerySpec([(DC, 0)], group_by=[2, 0], num_groups_limit=2600))
    # a matrix above PG_DISTINCT_GROUP_MAX_BYTES, from metadata alone: 5000 x 60 keys x (2^21 + 1 dictIds) bits = 78.6 GB
    n = 2049
    rng = np.random.default_rng(3)
    big = S.SegmentData("distinct_cap", n, [S.Column.from_dict_ids("big", np.arange((1 << 21) + 1, dtype=np.int32), rng.integers(0, (1 << 21) + 1, n).astype(np.int32)),
                                            S.Column.from_dict_ids("k1", np.arange(5000, dtype=np.int32), rng.integers(0, 5000, n).astype(np.int32)),
                                            S.Column.from_dict_ids("k2", np.arange(60, dtype=np.int32), rng.integers(0, 60, n).astype(np.int32))])
    with engine.open(big) as g:
        before = g.device_bytes()
        declined(g, Q.QuerySpec([(DC, 0)], group_by=[1, 2], num_groups_limit=300000), r"exceed PG_DISTINCT_GROUP_MAX_BYTES")
        assert g.device_bytes() == before          # nothing was allocated
        g.execute(Q.QuerySpec([(DC, 0)], group_by=[2]))
        assert g.device_bytes() > before           # the scratch belongs to the segment's contexts and is counted


def test_a_nullable_column_is_declined_under_null_handling_only(engine):
    n = 100003
    rng = np.random.default_rng(17)
    vals = rng.integers(0, 3000, n).astype(np.int32)
    nulls = rng.random(n) < 0.1
    with_nulls = vals.copy()
    with_nulls[nulls] = np.iinfo(np.int32).min
    seg = S.SegmentData("distinct_nulls", n, [S.Column.dict_encoded("vn", with_nulls).with_nulls(nulls), S.Column.dict_encoded("v", vals),
                                              S.Column.from_dict_ids("f", np.arange(100, dtype=np.int32), rng.integers(0, 100, n).astype(np.int32))])
    flt = Q.leaf(Q.Pred.dict_range(2, 0, 40))
    with engine.open(seg) as g:
        declined(g, Q.QuerySpec([(DC, 0)], filter=flt, null_handling=True), r"column vn, which carries a null value vector, under null handling")
        for spec in (Q.QuerySpec([(DC, 0)], filter=flt), Q.QuerySpec([(DC, 1), (Q.COUNT, -1)], filter=flt, null_handling=True)):
            got = g.execute(spec)
            D.assert_sets_equal(got, seg, spec)


def test_a_nullable_count_argument_keeps_the_scan_under_null_handling(engine):
    """AggregationPlanNode.java:98-115: hasNullValues (:130-153) looks at the argument of EVERY aggregation function, COUNT(column)'s included, so
    `DISTINCTCOUNT(v), COUNT(vn)` without a filter under null handling is scanned -- statistics (docs, 0, docs x 2, docs), the set of the dictIds
    that occur -- where the same query without null handling is answered from the dictionary (the whole dictionary, (docs, 0, 0, docs)).
    Found while the model of tests/fuzz_value_cases.py was written against the reference's rule; this is its smallest case."""
    n = 4099
    rng = np.random.default_rng(19)
    nulls = rng.random(n) < 0.1
    ids = rng.integers(0, 40, n).astype(np.int32) * 2          # the odd dictIds never occur
    seg = S.SegmentData("distinct_count_nulls", n, [S.Column.dict_encoded("vn", rng.integers(0, 30, n).astype(np.int32)).with_nulls(nulls),
                                                    S.Column.from_dict_ids("v", np.arange(80, dtype=np.int32), ids)])
    with engine.open(seg) as g:
        got = g.execute(Q.QuerySpec([(DC, 1), (Q.COUNT, 0)], null_handling=True))
        assert got.stats == (n, 0, 2 * n, n), got.stats
        assert np.array_equal(got.aggregations[0].dict_ids, np.unique(ids)) and got.aggregations[0].count == 40
        assert got.aggregations[1].count == n - int(nulls.sum())
        got = g.execute(Q.QuerySpec([(DC, 1), (Q.COUNT, 0)]))
        assert got.stats == (n, 0, 0, n), got.stats
        assert np.array_equal(got.aggregations[0].dict_ids, np.arange(80)) and got.aggregations[1].count == n


def test_a_typed_group_by_behind_an_index_leaf_sees_no_tiles_of_an_earlier_query(engine):
    """A GROUP BY that aggregates a raw DOUBLE column runs in group_typed_direct_kernel, which walks every tile and reads the index AND's bitmap
    there; the AND stores only the tiles that hold a match, so the others must be zeroed first -- they held what an earlier query of the same
    context had left, and numDocsScanned and the groups counted those docs too.  The smallest case of what tests/test_gpu_fuzz_values.py found
    (the ordinary query that brings a grouped DISTINCTCOUNT's statistics): query A's postings cover every tile, query B's only the first; B
    alone, after A, and A and B side by side in one pg_execute_batch."""
    n = 3 * 2048 + 5
    rng = np.random.default_rng(29)
    x = np.ones(n, dtype=np.int32)
    x[rng.permutation(2048)[:300]] = 0                      # dictId 0: 300 docs, all in the first tile
    k = rng.integers(0, 5, n).astype(np.int32)
    rd = rng.integers(-50, 50, n).astype(np.float64) * 0.25
    seg = S.SegmentData("distinct_index_tiles", n, [S.Column.from_dict_ids("x", np.arange(2, dtype=np.int32), x, with_inverted=True),
                                                    S.Column.from_dict_ids("k", np.arange(5, dtype=np.int32), k),
                                                    S.Column.raw_typed("rd", rd),
                                                    S.Column.from_dict_ids("v", np.arange(200, dtype=np.int32), rng.integers(0, 200, n).astype(np.int32))])
    leaf = lambda d: Q.leaf(Q.Pred.dict_range(0, d, d + 1, inverted=True))
    specs = {name: [Q.QuerySpec([(Q.COUNT, -1), (Q.MAX, 2)], filter=leaf(d), group_by=[1]), Q.QuerySpec([(DC, 3), (Q.MAX, 2)], filter=leaf(d), group_by=[1])]
             for name, d in (("a", 1), ("b", 0))}
    want = {name: oracle.execute(seg, pair[0]) for name, pair in specs.items()}
    assert want["a"].stats[0] == n - 300 and want["b"].stats[0] == 300

    def check(got, name, distinct):
        assert got.stats[0] == want[name].stats[0], (name, got.stats, want[name].stats)
        if distinct:
            D.assert_sets_equal(got, seg, specs[name][1])
            D.assert_other_functions_equal(got, seg, specs[name][1])
        else:
            H.assert_results_equal(got, want[name], check_stats=True)

    with engine.open(seg) as g:
        for _ in range(3):
            for name in ("a", "b"):
                for distinct in (0, 1):
                    check(g.execute(specs[name][distinct]), name, distinct)
        order = [("a", 0), ("b", 0), ("a", 1), ("b", 1)] * 6
        for _ in range(2):
            out = engine.execute_batch([g] * len(order), [specs[name][distinct] for name, distinct in order])
            for (status, got), (name, distinct) in zip(out, order):
                assert status == _abi.PG_OK
                check(got, name, distinct)


# ---- 9. the accessor ----
def test_the_accessor_rejects_what_is_not_a_set(engine, golden):
    seg, _ = golden
    ci = seg.column_index
    with engine.open(seg) as g:
        spec = Q.QuerySpec([(Q.COUNT, -1), (DC, ci("column1"))], filter=H.golden_filter(seg))
        for aggregation, row in ((-1, -1), (2, -1), (0, -1), (1, 0), (1, 1)):
            status, _, _ = raw_words(g, spec, aggregation, row)
            assert status == _abi.PG_ERR_INVALID_ARGUMENT, (aggregation, row)
        grouped = Q.QuerySpec([(DC, ci("column1"))], filter=H.golden_filter(seg), group_by=[ci("column9")])
        res = _abi.pg_result()
        _abi.check(g.lib, g.lib.pg_execute(g.handle, C.byref(grouped.c), C.byref(res)))
        try:
            words, n = C.POINTER(C.c_uint32)(), C.c_int32()
            for row in (-1, res.num_groups, res.num_groups + 7):
                assert g.lib.pg_result_distinct_dict_ids(C.byref(res), 0, row, C.byref(words), C.byref(n)) == _abi.PG_ERR_INVALID_ARGUMENT
            # the pointers stay valid until pg_result_free: read row 0 again after every other row was asked for
            assert g.lib.pg_result_distinct_dict_ids(C.byref(res), 0, 0, C.byref(words), C.byref(n)) == _abi.PG_OK
            first = np.ctypeslib.as_array(words, shape=(n.value,)).copy()
            keep = words
            for row in range(res.num_groups):
                w2, n2 = C.POINTER(C.c_uint32)(), C.c_int32()
                assert g.lib.pg_result_distinct_dict_ids(C.byref(res), 0, row, C.byref(w2), C.byref(n2)) == _abi.PG_OK
            assert np.array_equal(np.ctypeslib.as_array(keep, shape=(n.value,)), first)
        finally:
            g.lib.pg_result_free(C.byref(res))


def test_reserved_flag_bits_are_refused_at_every_entry(engine, golden):
    seg, _ = golden
    ci = seg.column_index
    with engine.open(seg) as g:
        for bit in (1 << 28, 1 << 29, 1 << 30):
            spec = Q.QuerySpec([(Q.COUNT, -1), (DC, ci("column1"))], filter=H.golden_filter(seg), group_by=[ci("column9")])
            spec.c.flags |= bit
            assert g.lib.pg_query_check(g.handle, C.byref(spec.c)) == _abi.PG_ERR_INVALID_ARGUMENT
            res = _abi.pg_result()
            assert g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res)) == _abi.PG_ERR_INVALID_ARGUMENT
            assert b"reserved bits" in g.lib.pg_last_error()
            g.lib.pg_result_free(C.byref(res))
            (status, _), = engine.execute_batch([g], [spec])
            assert status == _abi.PG_ERR_INVALID_ARGUMENT


# ---- the JNI function over the accessor, executed through the JVM stand-in ----
def test_the_native_method_returns_the_sets_with_the_result(engine, golden):
    from pinot_amd import jni_harness as J
    seg, _ = golden
    ci = seg.column_index
    jvm = J.FakeJvm()
    jvm.call("init", None, C.c_int32(0), C.c_int32(0))
    try:
        refs_before = jvm.lib.fj_live_refs()
        handle = jvm.segment_open(seg)
        try:
            for grouped in (False, True):
                spec = Q.QuerySpec([(Q.COUNT, -1), (DC, ci("column1")), (DC, ci("column3"))], filter=H.golden_filter_physical(seg), group_by=[ci("column9")] if grouped else [])
                assert jvm.query_check(handle, spec) == _abi.PG_OK
                result, sets = jvm.execute_with_distinct_sets(handle, spec)
                plain = jvm.execute(handle, spec)
                assert all(np.array_equal(a, b) for a, b in zip(result[1:], plain[1:])) and list(result[0][:4]) == list(plain[0][:4])
                want = D.model(seg, spec)
                group_ids = [int(x) for x in result[1]] if grouped else [None]
                rows = len(group_ids)
                assert len(sets) == 3 * rows and all(x is None for x in sets[:rows])
                for a in (1, 2):
                    for r, gid in enumerate(group_ids):
                        words = sets[a * rows + r].view(np.uint32)
                        ids = np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")).astype(np.int32)
                        assert np.array_equal(ids, want[gid][a] if grouped else want[a])
                        assert result[2][r * 3 + a] == len(ids)            # counts: the set's cardinality
                if not grouped:
                    assert (int(result[2][1]), int(result[2][2])) == (D.GOLDEN_ROWS["filter"]["v1"], D.GOLDEN_ROWS["filter"]["v2"])
        finally:
            jvm.call("segmentClose", None, C.c_int64(handle))
        assert jvm.lib.fj_live_refs() == refs_before
    finally:
        engine.reinit()
