"""Edges of the DISTINCTCOUNTHLL passes that random values do not reach (tests/hll_cases.py builds the segments):

  1. the constructed register corpus -- values whose hash was chosen by inverting Murmur2's hashLong: the first, a middle and the last
     register at log2m 4, 8 and 14, each with rank 1, 2, max - 1 and max = 32 - log2m + 1 (the remainder all zero: only the sentinel bit of
     hll_rank ends the count), the largest rank offered before AND after the smaller ones of its register, in runs a whole wavefront offers
     at once; raw and dictionary form, INT / LONG / FLOAT / DOUBLE; three register sizes side by side in one query;
  2. hll_fold_kernel's chunks -- dictionaries of 8191 ... 524289 entries with the first and the last dictId of every chunk set, chunks
     left wholly without a bit by the filter beside chunks that hold some, from the bitsets' LDS tier and from the HBM tier;
  3. scan_hll_kernel's LDS layout at the budget -- registers + the staged set area == the budget exactly runs, 4096 bytes more declines
     (and runs once the set area is not wanted); PG_HLL_GROUP_MAX_BYTES on both sides, from pg_query_check alone.

Registers are compared byte for byte with the numpy model over the docs oracle.filter_bitmap matches; nothing here has a tolerance."""
import numpy as np
import pytest

import distinct_cases as D
import hll_cases as HL
from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S
from test_gpu_hll import answered

pytestmark = pytest.mark.gpu


# ---- 1. the constructed register corpus ----
@pytest.mark.parametrize("raw", [True, False], ids=["raw", "dict"])
@pytest.mark.parametrize("num_docs", HL.CORPUS_SIZES)
def test_constructed_hashes_reach_the_first_and_last_register_with_the_largest_rank(engine, num_docs, raw):
    seg = HL.corpus_segment(S, num_docs, raw)
    flt = Q.leaf(Q.Pred.dict_range(HL.C_FILTER, 0, 900))
    with engine.open(seg) as g:
        for c in (HL.C_INT, HL.C_LONG, HL.C_FLOAT, HL.C_DOUBLE):
            aggs = [(Q.hll(4), c), (Q.hll(8), c), (Q.hll(14), c)]           # 64 + 1024 + 65536 bytes of registers side by side
            for name, spec in (("no filter", Q.QuerySpec(aggs)), ("range leaf", Q.QuerySpec(aggs + [(Q.COUNT, -1)], filter=flt)),
                               ("one key", Q.QuerySpec(aggs, group_by=[HL.C_KEY])), ("one key behind a range leaf", Q.QuerySpec(aggs, filter=flt, group_by=[HL.C_KEY]))):
                where = "%s n=%d column %d %s" % ("raw" if raw else "dict", num_docs, c, name)
                want = HL.model(seg, spec)
                if c in (HL.C_LONG, HL.C_DOUBLE) and not spec.group_by:
                    for a, log2m in enumerate(HL.CORPUS_LOG2M):
                        top = 32 - log2m + 1
                        assert want[a][0] == top and want[a][-1] == top and want[a].max() == top, (where, log2m)
                got = g.execute(spec)
                HL.assert_registers_equal(got, seg, spec, want=want, where=where)


# ---- 2. hll_fold_kernel's chunks ----
@pytest.fixture(scope="module")
def fold_segments():
    cache = {}

    def get(cardinality):
        if cardinality not in cache:
            cache[cardinality] = HL.fold_segment(S, cardinality)
        return cache[cardinality]
    return get


@pytest.mark.parametrize("tier", [None, "0"], ids=["tiers-by-size", "hbm-tier"])
@pytest.mark.parametrize("cardinality", HL.FOLD_CARDINALITIES)
def test_the_fold_reads_every_chunk_to_its_last_word(engine, fold_segments, cardinality, tier):
    seg = fold_segments(cardinality)
    chosen, chunk_of = HL.fold_dict_ids(cardinality)
    assert np.array_equal(np.unique(D.dict_ids_of(seg, HL.F_INT)), chosen)             # every chosen dictId is in some doc
    aggs = [(Q.hll(4), HL.F_INT), (Q.hll(14), HL.F_INT), (Q.hll(4), HL.F_LONG), (Q.hll(14), HL.F_LONG)]
    engine.reinit(PINOT_GPU_DISTINCT_LDS=tier)
    try:
        with engine.open(seg) as g:
            for name, (lo, hi) in (("every chunk", HL.FOLD_ALL), ("odd chunks only", HL.FOLD_ODD), ("even chunks only", HL.FOLD_EVEN)):
                for group_by in ([], [HL.F_KEY]):
                    spec = Q.QuerySpec(aggs, filter=Q.leaf(Q.Pred.dict_range(HL.F_FILTER, lo, hi)), group_by=group_by)
                    where = "cardinality %d %s%s" % (cardinality, name, " grouped" if group_by else "")
                    got = g.execute(spec)
                    HL.assert_registers_equal(got, seg, spec, where=where)
                    if not group_by and (lo, hi) == HL.FOLD_ALL:
                        assert got.stats[0] == seg.num_docs - 1
                        # every chosen dictId reached the registers: the model over the chosen dictionary entries alone is the same
                        for a, (f, c) in enumerate(aggs):
                            entries = np.asarray(seg.columns[c].dict_values)[chosen]
                            regs = HL.registers(entries, HL.numpy_dtype_of(seg.columns[c]), Q.hll_log2m(f))
                            assert np.array_equal(np.frombuffer(bytes(got.aggregations[a].hll_registers), dtype=np.uint8), regs), where
            if cardinality == 524289 and tier is None:
                # no filter: the host folds the whole dictionary, used by a doc or not (nothing is scanned)
                spec = Q.QuerySpec(aggs)
                got = g.execute(spec)
                assert got.stats == (seg.num_docs, 0, 0, seg.num_docs) and got.dominant_kernel_ms == 0.0
                want = {a: HL.registers(np.asarray(seg.columns[c].dict_values), HL.numpy_dtype_of(seg.columns[c]), Q.hll_log2m(f)) for a, (f, c) in enumerate(aggs)}
                HL.assert_registers_equal(got, seg, spec, want=want, where="the whole dictionary")
    finally:
        engine.reinit(PINOT_GPU_DISTINCT_LDS=None)


# ---- 3. scan_hll_kernel's LDS layout at the budget ----
LDS_BUDGET = _abi.PG_DISTINCT_LDS_MAX_DICT_IDS // 8                      # kLdsBudget (a static_assert in pg_engine.hip ties the two)
SET_AREA = _abi.PG_STAGED_SET_LDS_WORDS * 4                              # kSetLdsWords words (tied the same way)
FIT, OVER = (14, 14, 12, 10), (14, 14, 12, 11)
IN_LIST = list(range(0, 300, 7))
L_SET, L_RANGE = 4, 5


def lds_segment(num_docs):
    rng = np.random.default_rng(61 + num_docs)
    values = [rng.integers(-2 ** 31, 2 ** 31, num_docs).astype(np.int32) for _ in range(4)]
    cols = [S.Column.raw_typed("r%d" % i, v) for i, v in enumerate(values)]
    cols.append(S.Column.from_dict_ids("s", np.arange(300, dtype=np.int32) * 11, rng.integers(0, 300, num_docs).astype(np.int32)))
    cols.append(S.Column.from_dict_ids("flt", np.arange(1000, dtype=np.int32), rng.integers(0, 1000, num_docs).astype(np.int32)))
    seg = S.SegmentData("hll_lds_%d" % num_docs, num_docs, cols)
    for c, v in enumerate(values):
        HL.set_values(seg, c, v)
    return seg


@pytest.mark.parametrize("num_docs", [2049, 100003])
def test_registers_and_set_area_that_fill_the_lds_budget_exactly(engine, num_docs):
    registers = lambda slots: sum(4 << log2m for log2m in slots)
    assert len(IN_LIST) == 43 and registers(FIT) == 151552 and registers(FIT) + SET_AREA == LDS_BUDGET == 159744
    assert registers(OVER) + SET_AREA == 163840 and registers(OVER) <= LDS_BUDGET
    seg = lds_segment(num_docs)
    in_list = Q.leaf(Q.Pred.dict_set(L_SET, IN_LIST, 300))
    in_range = Q.leaf(Q.Pred.dict_range(L_RANGE, 0, 500))
    spec_of = lambda slots, flt: Q.QuerySpec([(Q.hll(log2m), c) for c, log2m in enumerate(slots)], filter=flt)
    declined = r"DISTINCTCOUNTHLL registers of %d bytes \(with the filter's set area\) exceed the %d bytes of LDS" % (registers(OVER) + SET_AREA, LDS_BUDGET)

    def runs(g, spec, where):
        got = g.execute(spec)
        HL.assert_registers_equal(got, seg, spec, where="n=%d %s" % (num_docs, where))
        assert got.dominant_kernel == "scan_hll_kernel", (where, got.dominant_kernel)
        assert got.stats[0] == int(D.matching_docs(seg, spec).sum()) and got.stats[2] == 4 * got.stats[0]

    cus = "1" if num_docs == 100003 else None                           # a grid sized for one CU: a wave walks many tiles
    engine.reinit(PINOT_GPU_TEST_CUS=cus)
    try:
        with engine.open(seg) as g:
            runs(g, spec_of(FIT, in_list), "the exact fit")
            answered(g, spec_of(OVER, in_list), _abi.PG_ERR_UNSUPPORTED, declined)
            runs(g, spec_of(OVER, in_range), "4096 bytes more behind a range leaf")
            engine.reinit(PINOT_GPU_SET_LDS="0")
            runs(g, spec_of(FIT, in_list), "the exact fit, sets in memory")
            runs(g, spec_of(OVER, in_list), "4096 bytes more, sets in memory")
    finally:
        engine.reinit(PINOT_GPU_SET_LDS=None, PINOT_GPU_TEST_CUS=None)


def test_the_group_cap_on_both_sides(engine):
    """PG_HLL_GROUP_MAX_BYTES from pg_query_check alone: nothing is allocated or executed.  128 x 128 raw group ids x one log2m-14 slot x 4
    bytes are exactly 2^30 -- not ABOVE the cap, so accepted; 129 x 128 decline.  (The default PINOT_GPU_GROUP_TABLE_BYTES budget is 64 GiB
    and does not bind below the cap.)"""
    import ctypes as C
    n = 2049
    rng = np.random.default_rng(67)
    key = lambda name, card: S.Column.from_dict_ids(name, np.arange(card, dtype=np.int32), rng.integers(0, card, n).astype(np.int32))
    seg = S.SegmentData("hll_cap_edges", n, [S.Column.raw_typed("v", rng.integers(-1000, 1000, n).astype(np.int32)), key("dv", 50),
                                             key("k128a", 128), key("k128b", 128), key("k129", 129)])
    assert 128 * 128 * (4 << 14) == _abi.PG_HLL_GROUP_MAX_BYTES
    with engine.open(seg) as g:
        before = g.device_bytes()
        for value in (0, 1):                                            # a raw value column, a dictionary one
            spec = Q.QuerySpec([(Q.hll(14), value)], group_by=[2, 3])
            status = g.lib.pg_query_check(g.handle, C.byref(spec.c))
            assert status == _abi.PG_OK, (value, status, (g.lib.pg_last_error() or b"").decode())
            spec = Q.QuerySpec([(Q.hll(14), value)], group_by=[4, 3])
            status = g.lib.pg_query_check(g.handle, C.byref(spec.c))
            message = (g.lib.pg_last_error() or b"").decode()
            assert status == _abi.PG_ERR_UNSUPPORTED, (value, status, message)
            assert "DISTINCTCOUNTHLL register matrices of %d bytes exceed PG_HLL_GROUP_MAX_BYTES (%d)" % (129 * 128 * (4 << 14), 1 << 30) in message, message
        assert g.device_bytes() == before
