"""PERCENTILE on dictionary columns on the device (PG_AGG_PERCENTILE, pg_result_percentile_counts), through the C ABI.

Expected values: the exact model of tests/percentile_cases.py (np.unique(..., return_counts=True) of the dictIds of the docs
oracle.filter_bitmap matches), the reference's own statistics and doubles (InterSegmentAggregationSingleValueQueriesTest.testPercentile
:379-473 over the committed fixture), and every other function of a mixed query against the unchanged oracle.  Lists are compared pair
for pair: there are no tolerances.

The two regimes (default, and PINOT_GPU_PERCENTILE_LDS=0: the counters in HBM at every cardinality) are switched with engine.reinit, which
makes the library read its environment again -- the way tests/test_gpu_distinct.py switches its tier."""
import ctypes as C
import re

import numpy as np
import pytest

import helpers as H
import percentile_cases as P
from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S

pytestmark = pytest.mark.gpu

SCAN = "scan_counts_kernel"
SWITCH = "PINOT_GPU_PERCENTILE_LDS"
PCT = Q.PERCENTILE
REGIMES = [None, "0"]


class regime:
    def __init__(self, engine, value):
        self.engine, self.value = engine, value

    def __enter__(self):
        self.engine.reinit(**{SWITCH: self.value})

    def __exit__(self, *exc):
        self.engine.reinit(**{SWITCH: None})


# ---- 1. the reference's goldens through the C ABI ----
@pytest.fixture(scope="module")
def golden():
    seg = H.golden_segment()
    return seg, {}          # the segment, and the models of its query shapes (computed once, shared, never changed)


def golden_model(golden, shape):
    seg, cache = golden
    if shape not in cache:
        cache[shape] = P.model(seg, P.golden_spec(seg, *P.GOLDEN_SHAPES[shape]))
    return cache[shape]


def check_golden(got, golden, shape, form="physical"):
    """The lists equal the model; the statistics are the reference's for ITS operator tree (H.golden_filter_physical); the same predicates
    as the logical tree are other iterator trees over the same docs, whose numEntriesScannedInFilter is the oracle's exact count."""
    from oracle import oracle
    seg, _ = golden
    filtered, grouped = P.GOLDEN_SHAPES[shape]
    spec = P.golden_spec(seg, filtered, grouped, form)
    row = P.GOLDEN_STATS[shape]
    entries = row[1] if (form == "physical" or not filtered) else oracle.execute(seg, P.without_percentile(spec)).stats[1]
    assert got.stats == (row[0], entries, row[2], row[3]) and got.filter_entries_exact, (got.stats, row, entries)
    want = golden_model(golden, shape)
    P.assert_counts_equal(got, seg, spec, want=want)
    # the sixteen doubles of the reference, from the lists the device returned (four copies of the segment multiply every count)
    for p in (50, 90, 95, 99):
        if grouped:
            lists = {g: {a: v[a].dict_id_counts for a in (0, 1)} for g, v in got.groups.items()}
            finals = max(P.golden_finals(seg, l, p) for l in lists.values())          # ORDER BY v1 DESC, v2 DESC LIMIT 1
        else:
            finals = P.golden_finals(seg, {a: got.aggregations[a].dict_id_counts for a in (0, 1)}, p)
        assert finals == P.GOLDEN_VALUES[(p, shape)], (p, shape, finals)


@pytest.mark.parametrize("shape", ["plain", "group"])
def test_goldens_without_a_filter_are_scanned(engine, golden, shape):
    seg, _ = golden
    with engine.open(seg) as g:
        got = g.execute(P.golden_spec(seg, *P.GOLDEN_SHAPES[shape]))
        check_golden(got, golden, shape)
        # no metadata fast path: the lists alone are one launch of the scan kernel; under GROUP BY the ordinary query's kernel and the pass's
        # are both in the result's time and either may be the longer one on 30 000 docs, so its kernel field is not asserted
        # (tools/kernel_coverage.py's trace is where group_counts_kernel is seen by name)
        if shape == "plain":
            assert got.dominant_kernel == SCAN


@pytest.mark.parametrize("form", ["logical", "inverted", "physical"])
@pytest.mark.parametrize("shape", ["filter", "filter+group"])
def test_goldens_under_the_filter_in_its_three_forms(engine, golden, shape, form):
    seg, _ = golden
    with engine.open(seg) as g:
        got = g.execute(P.golden_spec(seg, *P.GOLDEN_SHAPES[shape], form))
        check_golden(got, golden, shape, form)


def test_goldens_through_execute_batch_and_in_the_hbm_tier(engine, golden):
    seg, _ = golden
    shapes = ["plain", "filter", "filter+group"]
    with engine.open(seg) as g:
        specs = [P.golden_spec(seg, *P.GOLDEN_SHAPES[s], "physical") for s in shapes]
        for shape, (status, got) in zip(shapes, engine.execute_batch([g] * 3, specs)):
            assert status == _abi.PG_OK
            check_golden(got, golden, shape)
    with regime(engine, "0"):
        with engine.open(seg) as g:
            for shape in shapes + ["group"]:
                check_golden(g.execute(P.golden_spec(seg, *P.GOLDEN_SHAPES[shape], "physical")), golden, shape)


# ---- 2. the tiers ----
TIER_CARDS = [1, 33, 257, 5000]
TIER_DOCS = 2048 * 5 + 37          # the last tile is partial


@pytest.fixture(scope="module")
def tier_segment():
    seg = P.synthetic_segment(S, "percentile_tiers", TIER_DOCS, TIER_CARDS + [1000, 50, 40, 13])
    n = seg.num_docs
    rng = np.random.default_rng(77)
    # two columns with postings for the index-driven filter, one value column for the SUM beside the lists
    extra = [S.Column.from_dict_ids("x", np.arange(50, dtype=np.int32), rng.integers(0, 50, n).astype(np.int32), with_inverted=True),
             S.Column.from_dict_ids("y", np.arange(40, dtype=np.int32), rng.integers(0, 40, n).astype(np.int32), with_inverted=True)]
    return S.SegmentData("percentile_tiers", n, list(seg.columns) + extra)


def tier_filters():
    f, s, x, y = 4, 7, 8, 9
    return {
        "none": None,
        "range": Q.leaf(Q.Pred.dict_range(f, 0, 700)),
        "set": Q.leaf(Q.Pred.dict_set(s, [1, 5, 11], 13)),
        "tree": Q.or_(Q.leaf(Q.Pred.dict_range(f, 0, 100)), Q.not_(Q.leaf(Q.Pred.dict_set(s, [0, 2, 3, 4, 6, 7, 8, 9, 10, 12], 13)))),
        "index": Q.and_(Q.leaf(Q.Pred.dict_range(x, 3, 9, inverted=True)), Q.leaf(Q.Pred.dict_range(y, 5, 20, inverted=True)), Q.leaf(Q.Pred.dict_range(f, 0, 500))),
    }


@pytest.mark.parametrize("lds", REGIMES)
@pytest.mark.parametrize("flt", ["none", "range", "set", "tree", "index"])
def test_tiers_columns_and_filters(engine, tier_segment, flt, lds):
    seg = tier_segment
    with regime(engine, lds):
        with engine.open(seg) as g:
            for num_cols in (1, 2, 3, 4):
                # rotate so that every cardinality is the first column once
                cols = [(num_cols - 1 + i) % 4 for i in range(num_cols)]
                spec = Q.QuerySpec([(PCT, c) for c in cols] + [(Q.COUNT, -1), (Q.SUM, 4)], filter=tier_filters()[flt])
                got = g.execute(spec)
                P.assert_counts_equal(got, seg, spec, where="%s cols %r" % (flt, cols))
                P.assert_other_functions_equal(got, seg, spec)
            # the lists alone: one launch that counts the docs and the filter entries itself
            spec = Q.QuerySpec([(PCT, 3), (PCT, 1), (Q.COUNT, -1)], filter=tier_filters()[flt])
            got = g.execute(spec)
            P.assert_counts_equal(got, seg, spec)
            P.assert_other_functions_equal(got, seg, spec)
            assert got.aggregations[2].count == got.stats[0] == got.aggregations[0].count
            assert got.dominant_kernel == SCAN or (flt == "index" and got.dominant_kernel == "index_and_kernel")          # (the index intersection may outlast the scan of its few tiles)


# ---- 3. the tier boundary: the engine's own arithmetic (include/pinot_gpu.h PG_PERCENTILE_LDS_MAX_COUNTERS, checked against
# kLdsBudget - the reduction records by a static_assert in pg_engine.hip; a staged filter set takes kSetLdsWords = 2048 more) ----
@pytest.fixture(scope="module")
def boundary_segment():
    reach = _abi.PG_PERCENTILE_LDS_MAX_COUNTERS
    a = 20000
    # c0 + c1 = reach (fits), c0 + c2 = reach + 1 (does not); c3: a filter column; c4: a 13-value column for a staged set
    return P.synthetic_segment(S, "percentile_boundary", 100003, [a, reach - a, reach - a + 1, 1000, 13], last_present=True)


def test_the_tier_boundary_follows_the_lds_budget(engine, boundary_segment):
    seg = boundary_segment
    reach = _abi.PG_PERCENTILE_LDS_MAX_COUNTERS
    assert seg.columns[0].cardinality + seg.columns[1].cardinality == reach == seg.columns[0].cardinality + seg.columns[2].cardinality - 1
    rng_filter = Q.leaf(Q.Pred.dict_range(3, 0, 600))
    with engine.open(seg) as g:
        seen = {}
        for name, cols, flt in (("under", (0, 1), rng_filter), ("over", (0, 2), rng_filter)):
            spec = Q.QuerySpec([(PCT, c) for c in cols], filter=flt)
            got = g.execute(spec)
            assert got.dominant_kernel == SCAN
            P.assert_counts_equal(got, seg, spec, where=name)
            for a, c in enumerate(cols):
                assert got.aggregations[a].dict_id_counts[0][-1] <= seg.columns[c].cardinality - 1
            seen[name] = got
        # the highest dictId of every column occurs in the segment: without a filter it is counted in either tier
        for cols in ((0, 1), (0, 2)):
            spec = Q.QuerySpec([(PCT, c) for c in cols])
            got = g.execute(spec)
            P.assert_counts_equal(got, seg, spec)
            assert [int(got.aggregations[a].dict_id_counts[0][-1]) for a in range(2)] == [seg.columns[c].cardinality - 1 for c in cols]
        # pg_result's kernel field names the kernel; both tiers are instantiations of scan_counts_kernel and share PG_KERNEL_SCAN_COUNTS (the
        # two instantiations are told apart by name in the kernel-coverage gate's trace, which requires both to have run)
        assert seen["under"].dominant_kernel == seen["over"].dominant_kernel == SCAN
    with regime(engine, "0"):
        with engine.open(seg) as g:
            spec = Q.QuerySpec([(PCT, 0), (PCT, 1)], filter=rng_filter)
            P.assert_counts_equal(g.execute(spec), seg, spec)


# ---- 3b. the set area beside the counters: both sides of every edge of scan_grid's arithmetic.  counters (rounded up to 16 bytes) + the staged
# set area (kSetLdsWords = 2048 words, when the filter has a dictId-set leaf and PINOT_GPU_SET_LDS is on) + the reduction records <= kLdsBudget:
#   R - K      the set is staged behind the counters and the three add up to the budget exactly;
#   R - K + 1  the set no longer fits beside the counters: it stays in memory, the counters stay in LDS;
#   R          the counters alone fit exactly;      R + 1  the HBM tier.
# Which branch ran is not visible from outside (one kernel id): the test holds the answer on both sides of every edge, with the HIGHEST dictId of
# every PERCENTILE column among the matching docs -- an area that overlaps the last counters shows there and nowhere else.
EDGE_K = 2048
EDGE_A = 20000
EDGE_SET_CARDS = {"13 values": 13, "65536: the set fills the area": 65536, "65537: 17 bits, never staged": 65537}


@pytest.fixture(scope="module")
def set_edge_segment():
    r, n = _abi.PG_PERCENTILE_LDS_MAX_COUNTERS, 100003
    rng = np.random.default_rng(41)
    # columns 0-4: PERCENTILE columns; 0 + 1 = R - K, 0 + 2 = R - K + 1, 0 + 3 = R, 0 + 4 = R + 1.  columns 5-7: the set-leaf columns.
    cards = [EDGE_A, r - EDGE_K - EDGE_A, r - EDGE_K - EDGE_A + 1, r - EDGE_A, r - EDGE_A + 1] + list(EDGE_SET_CARDS.values())
    ids = [rng.integers(0, card, n).astype(np.int32) for card in cards]
    members = {c: (0, cards[c] // 2, cards[c] - 1) for c in (5, 6, 7)}
    # docs that carry the highest dictId of PERCENTILE column j AND a member of every IN list (lowest, middle, highest in turn): in the first tile,
    # in a middle tile and in the last, partial, tile
    for j in range(5):
        for t, doc in enumerate((7 + 64 * j, 2048 * 23 + 100 + j, n - 1 - j)):
            ids[j][doc] = cards[j] - 1
            for c in (5, 6, 7):
                ids[c][doc] = members[c][(j + t) % 3]
    cols = [S.Column.from_dict_ids("c%d" % i, (np.arange(card, dtype=np.int64) * 3 - card).astype(np.int32), ids[i]) for i, card in enumerate(cards)]
    seg = S.SegmentData("percentile_set_edges", n, cols)
    seg.members = members
    return seg


@pytest.mark.parametrize("set_lds", [None, "0"], ids=["sets-staged", "PINOT_GPU_SET_LDS=0"])
def test_the_set_area_beside_the_counters_on_both_sides_of_every_edge(engine, set_edge_segment, set_lds):
    from oracle import oracle
    seg = set_edge_segment
    r = _abi.PG_PERCENTILE_LDS_MAX_COUNTERS
    totals = {1: r - EDGE_K, 2: r - EDGE_K + 1, 3: r, 4: r + 1}
    engine.reinit(PINOT_GPU_SET_LDS=set_lds)
    try:
        with engine.open(seg) as g:
            for other, total in totals.items():
                assert seg.columns[0].cardinality + seg.columns[other].cardinality == total
                for set_col in (5, 6, 7):
                    card = seg.columns[set_col].cardinality
                    assert seg.columns[set_col].bits == (4 if card == 13 else (16 if card == 65536 else 17))
                    # the IN list leads a small tree once (a second node beside it: the staged set of a tree, not of a single leaf)
                    leaf = Q.leaf(Q.Pred.dict_set(set_col, list(seg.members[set_col]), card))
                    for flt in (leaf, Q.or_(leaf, Q.leaf(Q.Pred.dict_range(0, EDGE_A - 1, EDGE_A)))):
                        spec = Q.QuerySpec([(PCT, 0), (PCT, other), (Q.COUNT, -1)], filter=flt)
                        where = "total %d, set column of %d" % (total, card)
                        got = g.execute(spec)
                        assert got.dominant_kernel == SCAN, where
                        P.assert_counts_equal(got, seg, spec, where=where)
                        for a, c in enumerate((0, other)):
                            assert int(got.aggregations[a].dict_id_counts[0][-1]) == seg.columns[c].cardinality - 1, where
                        want = oracle.execute(seg, P.without_percentile(spec))
                        assert got.aggregations[2].count == want.aggregations[2].count == got.stats[0] == got.aggregations[0].count > 0, where
                        P.assert_other_functions_equal(got, seg, spec)
    finally:
        engine.reinit(PINOT_GPU_SET_LDS=None)


# ---- 4. skew ----
@pytest.mark.parametrize("lds", REGIMES)
def test_every_doc_on_one_dict_id_and_a_filter_that_matches_nothing(engine, lds):
    n = 300000
    rng = np.random.default_rng(5)
    seg = S.SegmentData("percentile_skew", n, [S.Column.from_dict_ids("same", np.arange(5000, dtype=np.int32) * 3, np.full(n, 77, dtype=np.int32)),
                                               S.Column.from_dict_ids("f", np.arange(1000, dtype=np.int32), rng.integers(0, 1000, n).astype(np.int32))])
    with regime(engine, lds):
        with engine.open(seg) as g:
            got = g.execute(Q.QuerySpec([(PCT, 0)]))
            ids, counts = got.aggregations[0].dict_id_counts
            assert list(ids) == [77] and list(counts) == [n] and got.aggregations[0].count == n          # above any 8- or 16-bit field
            assert got.stats == (n, 0, n, n) and got.dominant_kernel == SCAN
            nothing = Q.and_(Q.leaf(Q.Pred.dict_range(1, 0, 10)), Q.leaf(Q.Pred.dict_range(1, 500, 510)))
            got = g.execute(Q.QuerySpec([(PCT, 0), (Q.COUNT, -1)], filter=nothing))
            ids, counts = got.aggregations[0].dict_id_counts
            assert len(ids) == 0 and len(counts) == 0 and got.aggregations[0].count == 0 and got.aggregations[1].count == 0
            assert P.percentile_of_counts(P.values_of(seg, 0, ids), counts, 50) == float("-inf")
            res = _abi.pg_result()
            spec = Q.QuerySpec([(PCT, 0)], filter=nothing)
            _abi.check(g.lib, g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res)))
            try:
                pi, pc, num = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint32)(), C.c_int32(-1)
                assert g.lib.pg_result_percentile_counts(C.byref(res), 0, -1, C.byref(pi), C.byref(pc), C.byref(num)) == _abi.PG_OK and num.value == 0
            finally:
                g.lib.pg_result_free(C.byref(res))


# ---- 5. the same column twice ----
def test_the_same_column_twice_shares_one_vector(engine, tier_segment):
    seg = tier_segment
    spec = Q.QuerySpec([(PCT, 3), (Q.COUNT, -1), (PCT, 3)], filter=Q.leaf(Q.Pred.dict_range(4, 0, 300)))          # PERCENTILE50(c), PERCENTILE99(c)
    with engine.open(seg) as g:
        got = g.execute(spec)
        P.assert_counts_equal(got, seg, spec)
        a, b = got.aggregations[0].dict_id_counts, got.aggregations[2].dict_id_counts
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert got.stats[2] == got.stats[0] * 1          # the column is projected once


# ---- 6. GROUP BY ----
@pytest.fixture(scope="module")
def group_segment():
    n = 20003
    rng = np.random.default_rng(31)
    ids = lambda card: rng.integers(0, card, n).astype(np.int32)
    key_raw = rng.integers(-40, 60, n).astype(np.int32)
    cols = [S.Column.from_dict_ids("k3", np.arange(3, dtype=np.int32), ids(3)),                             # 0
            S.Column.from_dict_ids("k5", np.arange(5, dtype=np.int32) * 7, ids(5)),                         # 1
            S.Column.from_dict_ids("k40", np.arange(40, dtype=np.int32), ids(40)),                          # 2
            S.Column.from_dict_ids("v", (np.arange(257, dtype=np.int64) * 7 + 3).astype(np.int32), ids(257)),   # 3
            S.Column.from_dict_ids("w", np.arange(5000, dtype=np.int32), ids(5000)),                        # 4
            S.Column.from_dict_ids("f", np.arange(1000, dtype=np.int32), ids(1000)),                        # 5
            S.Column.raw("kr", key_raw)]                                                                    # 6: raw INT key
    seg = S.SegmentData("percentile_groups", n, cols)
    seg.key_raw = key_raw
    return seg


def check_mix(g, seg, spec, key_values=None):
    got = g.execute(spec)
    P.assert_counts_equal(got, seg, spec, key_values=key_values)
    P.assert_other_functions_equal(got, seg, spec)
    return got


@pytest.mark.parametrize("lds", REGIMES)
def test_group_by_dictionary_keys_a_raw_key_and_emptied_groups(engine, group_segment, lds):
    seg = group_segment
    f_lt = lambda t: Q.leaf(Q.Pred.dict_range(5, 0, t))
    with regime(engine, lds):
        with engine.open(seg) as g:
            got = check_mix(g, seg, Q.QuerySpec([(PCT, 3), (Q.SUM, 3), (PCT, 4)], filter=f_lt(400), group_by=[2]))          # 40
            assert got.group_id_upper_bound == 40
            got = check_mix(g, seg, Q.QuerySpec([(PCT, 4), (Q.SUM, 3)], filter=f_lt(700), group_by=[0, 1]))                 # 3 x 5
            assert got.group_id_upper_bound == 15
            # groups the filter empties are absent: only k5 in {1, 3} survives
            got = check_mix(g, seg, Q.QuerySpec([(PCT, 3)], filter=Q.leaf(Q.Pred.dict_set(1, [1, 3], 5)), group_by=[0, 1]))
            assert len(got.groups) == 6 and all((gid // 3) in (1, 3) for gid in got.groups)
            # one raw INT key, keyed by offset
            base, is_offset, _ = g.group_key_info(6)
            assert is_offset == 1
            kv = {6: (seg.key_raw, base, int(seg.key_raw.max()) - int(seg.key_raw.min()) + 1)}
            check_mix(g, seg, Q.QuerySpec([(PCT, 3), (Q.COUNT, -1)], filter=f_lt(250), group_by=[6]), key_values=kv)


# ---- 7. declines ----
def declined(g, spec, pattern, status_want=_abi.PG_ERR_UNSUPPORTED):
    for check in (True, False):
        if check:
            status = g.lib.pg_query_check(g.handle, C.byref(spec.c))
        else:
            res = _abi.pg_result()
            status = g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res))
            g.lib.pg_result_free(C.byref(res))
        message = (g.lib.pg_last_error() or b"").decode()
        assert status == status_want, (status, message)
        assert re.search(pattern, message), message


@pytest.fixture(scope="module")
def decline_segment():
    n = 4099
    rng = np.random.default_rng(9)
    ids = lambda card: rng.integers(0, card, n).astype(np.int32)
    cols = [S.Column.from_dict_ids("a", np.arange(200, dtype=np.int32), ids(200)),        # 0
            S.Column.from_dict_ids("b", np.arange(13, dtype=np.int32), ids(13)),          # 1
            S.Column.from_dict_ids("c", np.arange(5000, dtype=np.int32), ids(5000)),      # 2
            S.Column.from_dict_ids("d", np.arange(1000, dtype=np.int32), ids(1000)),      # 3
            S.Column.from_dict_ids("e", np.arange(100000, dtype=np.int32), ids(100000)),  # 4
            S.Column.from_dict_ids("f", np.arange(33, dtype=np.int32), ids(33)),          # 5
            S.Column.raw("r", rng.integers(0, 1000, n).astype(np.int32)),                 # 6: raw INT
            S.Column.raw_typed("rl", rng.integers(0, 1 << 40, n).astype(np.int64))]             # 7: raw LONG
    return S.SegmentData("percentile_declines", n, cols)


def test_declines_name_their_reason(engine, decline_segment):
    seg = decline_segment
    with engine.open(seg) as g:
        declined(g, Q.QuerySpec([(PCT, 6)]), r"PERCENTILE on raw \(no-dictionary\) column r\b")
        declined(g, Q.QuerySpec([(PCT, c) for c in (0, 1, 2, 3, 5)]), r"more than 4 PERCENTILE columns")
        declined(g, Q.QuerySpec([(PCT, 0)], filter=Q.leaf(Q.Pred.raw_range(7, 0, 1 << 30))), r"PERCENTILE beside a range predicate on raw LONG / FLOAT / DOUBLE column rl")
        declined(g, Q.QuerySpec([(PCT, 0), (Q.DISTINCTCOUNT, 1)]), r"PERCENTILE beside DISTINCTCOUNT")
        declined(g, Q.QuerySpec([(Q.DISTINCTCOUNT, 1), (Q.COUNT, -1), (PCT, 0)]), r"PERCENTILE beside DISTINCTCOUNT")
        # GROUP BY outside plan_distinct's conditions
        declined(g, Q.QuerySpec([(PCT, 0)], group_by=[4, 2, 3, 0]), r"key space of kind 1")
        declined(g, Q.QuerySpec([(PCT, 0)], group_by=[2, 3]), r"above numGroupsLimit 100000")
        declined(g, Q.QuerySpec([(PCT, 0)], group_by=[1, 0], num_groups_limit=2599), r"above numGroupsLimit 2599")
        declined(g, Q.QuerySpec([(PCT, 0)], group_by=[1, 0, 5, 1, 5]), r"more than 4 group-by columns")
        # the byte limit, by arithmetic on a group space too large to allocate: 5000 x 13 keys x 100000 counters x 4 bytes = 26 GB
        before = g.device_bytes()
        declined(g, Q.QuerySpec([(PCT, 4)], group_by=[2, 1]), r"PERCENTILE counter matrices of \d+ bytes exceed PG_PERCENTILE_GROUP_MAX_BYTES")
        assert g.device_bytes() == before          # nothing was allocated
        # 1000 x 13 keys x (100000 counters + the 31073 behind the last: 2^17 - 100000 + 1) x 4 bytes: the message states the sum
        g.lib.pg_query_check(g.handle, C.byref(Q.QuerySpec([(PCT, 4)], group_by=[3, 1]).c))
        want = 13000 * 100000 * 4 + ((1 << 17) - 100000 + 1) * 4
        assert ("matrices of %d bytes" % want) in g.lib.pg_last_error().decode()
        g.execute(Q.QuerySpec([(PCT, 0)], group_by=[1, 0], num_groups_limit=2600))
        assert g.device_bytes() > before           # the scratch belongs to the segment's contexts and is counted


def test_a_nullable_column_is_declined_under_null_handling_only(engine):
    n = 10007
    rng = np.random.default_rng(17)
    vals = rng.integers(0, 3000, n).astype(np.int32)
    nulls = rng.random(n) < 0.1
    with_nulls = vals.copy()
    with_nulls[nulls] = np.iinfo(np.int32).min
    seg = S.SegmentData("percentile_nulls", n, [S.Column.dict_encoded("vn", with_nulls).with_nulls(nulls), S.Column.dict_encoded("v", vals),
                                                S.Column.from_dict_ids("f", np.arange(100, dtype=np.int32), rng.integers(0, 100, n).astype(np.int32))])
    flt = Q.leaf(Q.Pred.dict_range(2, 0, 40))
    with engine.open(seg) as g:
        declined(g, Q.QuerySpec([(PCT, 0)], filter=flt, null_handling=True), r"PERCENTILE on column vn, which carries a null value vector, under null handling")
        for spec in (Q.QuerySpec([(PCT, 0)], filter=flt), Q.QuerySpec([(PCT, 1), (Q.COUNT, -1)], filter=flt, null_handling=True)):
            P.assert_counts_equal(g.execute(spec), seg, spec)


def test_the_internal_flag_bit_is_refused_from_callers(engine, decline_segment):
    seg = decline_segment
    with engine.open(seg) as g:
        spec = Q.QuerySpec([(Q.COUNT, -1), (PCT, 0)], filter=Q.leaf(Q.Pred.dict_range(3, 0, 500)))
        spec.c.flags |= 1 << 27
        declined(g, spec, r"reserved bits", status_want=_abi.PG_ERR_INVALID_ARGUMENT)
        (status, _), = engine.execute_batch([g], [spec])
        assert status == _abi.PG_ERR_INVALID_ARGUMENT


# ---- 8. the accessor ----
def test_the_accessor_rejects_what_is_not_a_list(engine, decline_segment):
    seg = decline_segment
    flt = Q.leaf(Q.Pred.dict_range(3, 0, 500))

    def ask(res, aggregation, row):
        pi, pc, num = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint32)(), C.c_int32(-1)
        status = g.lib.pg_result_percentile_counts(C.byref(res), aggregation, row, C.byref(pi), C.byref(pc), C.byref(num))
        return status, pi, pc, num.value

    with engine.open(seg) as g:
        spec = Q.QuerySpec([(Q.COUNT, -1), (PCT, 0), (Q.SUM, 2)], filter=flt)
        res = _abi.pg_result()
        _abi.check(g.lib, g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res)))
        try:
            for aggregation, row in ((-1, -1), (3, -1), (0, -1), (2, -1), (1, 0), (1, 1)):
                assert ask(res, aggregation, row)[0] == _abi.PG_ERR_INVALID_ARGUMENT, (aggregation, row)
            status, pi, pc, num = ask(res, 1, -1)
            assert status == _abi.PG_OK and num > 0
            ids = np.ctypeslib.as_array(pi, shape=(num,))
            counts = np.ctypeslib.as_array(pc, shape=(num,))
            assert (np.diff(ids) > 0).all() and (counts > 0).all() and int(counts.sum()) == res.aggregations[1].count
        finally:
            g.lib.pg_result_free(C.byref(res))
        grouped = Q.QuerySpec([(PCT, 0)], filter=flt, group_by=[1])
        res = _abi.pg_result()
        _abi.check(g.lib, g.lib.pg_execute(g.handle, C.byref(grouped.c), C.byref(res)))
        try:
            for row in (-1, res.num_groups, res.num_groups + 7):
                assert ask(res, 0, row)[0] == _abi.PG_ERR_INVALID_ARGUMENT
            # the pointers stay valid until pg_result_free: read row 0 again after every other row was asked for
            status, pi, pc, num = ask(res, 0, 0)
            assert status == _abi.PG_OK
            first = np.ctypeslib.as_array(pc, shape=(num,)).copy()
            for row in range(res.num_groups):
                assert ask(res, 0, row)[0] == _abi.PG_OK
            assert np.array_equal(np.ctypeslib.as_array(pc, shape=(num,)), first)
        finally:
            g.lib.pg_result_free(C.byref(res))


# ---- 9. the reference's goldens through SQL: the host mirror over four copies of the segment (testPercentile :379-473, its SQL verbatim) ----
SQL_FILTER = (" WHERE column1 > 100000000 AND column3 BETWEEN 20000000 AND 1000000000 AND column5 = 'gFuH'"
              " AND (column6 < 500000000 OR column11 NOT IN ('t', 'P')) AND daysSinceEpoch = 126164076")
SQL_GROUP_BY = " GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1"
SQL_SHAPES = {"plain": ("", (120000, 0, 240000, 120000)), "filter": (SQL_FILTER, (24516, 252256, 49032, 120000)),
              "group": (SQL_GROUP_BY, (120000, 0, 360000, 120000)), "filter+group": (SQL_FILTER + SQL_GROUP_BY, (24516, 252256, 73548, 120000))}
SQL_QUERIES = [(50, "SELECT PERCENTILE50(column1) AS v1, PERCENTILE50(column3) AS v2 FROM testTable"),
               (50, "SELECT PERCENTILE(column1, 50) AS v1, PERCENTILE(column3, 50) AS v2 FROM testTable"),
               (50, "SELECT PERCENTILE(column1, '50') AS v1, PERCENTILE(column3, '50') AS v2 FROM testTable"),
               (90, "SELECT PERCENTILE90(column1) AS v1, PERCENTILE90(column3) AS v2 FROM testTable"),
               (95, "SELECT PERCENTILE95(column1) AS v1, PERCENTILE95(column3) AS v2 FROM testTable"),
               (99, "SELECT PERCENTILE99(column1) AS v1, PERCENTILE99(column3) AS v2 FROM testTable")]


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


@pytest.mark.parametrize("shape", ["plain", "filter", "group", "filter+group"])
@pytest.mark.parametrize("query", range(len(SQL_QUERIES)))
def test_goldens_through_sql_over_four_segments(golden_host_segments, query, shape):
    from pinot_amd import host
    p, select = SQL_QUERIES[query]
    tail, stats = SQL_SHAPES[shape]
    sql = select + tail
    out = host.execute_sql(golden_host_segments, sql, max_execution_threads=4)
    st = out["combined"]["stats"]
    assert (st["numDocsScanned"], st["numEntriesScannedInFilter"], st["numEntriesScannedPostFilter"], st["numTotalDocs"]) == stats, sql
    want = list(P.GOLDEN_VALUES[(p, shape)])
    if "GROUP BY" in sql:
        assert out["resultTable"]["rows"] == [want], sql
    else:
        assert out["combined"]["final"] == want, sql
        # the combined list holds four copies of a segment's: its length is the docs scanned
        assert [sum(v["counts"]) for v in out["combined"]["intermediate"]] == [stats[0], stats[0]]


def test_what_keeps_the_cpu_plan_on_the_sql_path(golden_host_segments):
    from pinot_amd import host
    with pytest.raises(host.HostError) as e:
        host.execute_sql_datatable(golden_host_segments[:1], SQL_QUERIES[0][1] + SQL_FILTER)
    assert e.value.status == 2 and "PERCENTILE" in str(e.value)
    # FILTER (WHERE ...) beside it, and a STRING column
    for sql in ("SELECT PERCENTILE50(column1), COUNT(*) FILTER (WHERE column1 > 100000000) FROM testTable", "SELECT PERCENTILE50(column5) FROM testTable"):
        with pytest.raises(host.HostError) as e:
            host.execute_sql(golden_host_segments[:1], sql)
        assert e.value.status == 2, sql


# ---- 10. the JNI function over the accessor, executed through the JVM stand-in ----
def test_the_native_method_returns_the_lists_with_the_result(engine, golden):
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
                spec = Q.QuerySpec([(Q.COUNT, -1), (PCT, ci("column1")), (PCT, ci("column3"))], filter=H.golden_filter_physical(seg), group_by=[ci("column9")] if grouped else [])
                assert jvm.query_check(handle, spec) == _abi.PG_OK
                result, ids, counts = jvm.execute_with_percentile_counts(handle, spec)
                plain = jvm.execute(handle, spec)
                assert all(np.array_equal(a, b) for a, b in zip(result[1:], plain[1:])) and list(result[0][:4]) == list(plain[0][:4])
                want = P.model(seg, spec)
                group_ids = [int(x) for x in result[1]] if grouped else [None]
                rows = len(group_ids)
                assert len(ids) == len(counts) == 3 * rows and all(x is None for x in ids[:rows]) and all(x is None for x in counts[:rows])
                for a in (1, 2):
                    for r, gid in enumerate(group_ids):
                        pairs = want[gid][a] if grouped else want[a]
                        assert np.array_equal(np.asarray(ids[a * rows + r]).view(np.int32), pairs[0])
                        assert np.array_equal(np.asarray(counts[a * rows + r]).view(np.uint32), pairs[1])
                        assert result[2][r * 3 + a] == int(pairs[1].astype(np.int64).sum())            # counts: the docs aggregated
                # the arrays equal the C ABI's
                got = None
                with engine.open(seg) as g:
                    got = g.execute(spec)
                for a in (1, 2):
                    for r, gid in enumerate(group_ids):
                        v = got.groups[gid][a] if grouped else got.aggregations[a]
                        assert np.array_equal(np.asarray(ids[a * rows + r]).view(np.int32), v.dict_id_counts[0])
                        assert np.array_equal(np.asarray(counts[a * rows + r]).view(np.uint32), v.dict_id_counts[1])
        finally:
            jvm.call("segmentClose", None, C.c_int64(handle))
        assert jvm.lib.fj_live_refs() == refs_before
    finally:
        engine.reinit()
