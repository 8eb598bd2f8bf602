"""GPU tests of scan_simple_dma_pair_kernel<FB, VB, aux> (pinot_amd/csrc/pg_scan_simple_dma.h): the ring kernel with both widths as compile-time
constants -- constant staging, every dword of the lane read once at the top of the tile, no width switch, the launch's uniform branches taken
around the tile loop -- instantiated for the 102 width pairs the rule admits (pg_dma_pairs.h: 27 <= f.bits + v.bits <= 38, both up to 20).

Every query runs four ways on one open segment: the pair kernel (PINOT_GPU_SCAN_SIMPLE_DMA=2), the generic ring kernel
(PINOT_GPU_SCAN_SIMPLE_DMA_PAIR=0 beside it), no ring at all (PINOT_GPU_SCAN_SIMPLE_DMA=0) and the oracle; all four are bit equal and every
kernel reports `scan_simple_kernel`.  That each instance is dispatched is the coverage gate's to show (tools/kernel_coverage.py `pair-F-V-ntA`).

Shapes: one compute unit with one workgroup of four waves, so that wave w owns tiles w, w + 4, ...: 3, 6 and 11 tiles give waves with 0 and 1,
1 and 2, 2 and 3 tiles (prologue only, one pass of the loop, the loop and the drain), each ending on a partial tile."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle
from pinot_amd import query as Q
from pinot_amd import segment as S
import helpers as H

pytestmark = pytest.mark.gpu

DMA, PAIR, NT, BPC = ("PINOT_GPU_SCAN_SIMPLE_DMA", "PINOT_GPU_SCAN_SIMPLE_DMA_PAIR", "PINOT_GPU_SCAN_SIMPLE_DMA_NT",
                      "PINOT_GPU_SCAN_SIMPLE_DMA_BLOCKS_PER_CU")
WAYS = {"pair": {DMA: "2", PAIR: None}, "generic": {DMA: "2", PAIR: "0"}, "no-ring": {DMA: "0", PAIR: None}}
ADMITTED = [(f, v) for f in range(1, 21) for v in range(1, 21) if 27 <= f + v <= 38]
EXTREMES = [(10, 17), (7, 20), (20, 7), (18, 20), (20, 18)]
EVERY_FUNCTION = [(Q.COUNT, -1), (Q.SUM, 1), (Q.MIN, 1), (Q.MAX, 1), (Q.AVG, 1)]


def test_the_admitted_pairs_are_the_header_s():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pinot_amd", "csrc", "pg_dma_pairs.h")).read()
    assert len(ADMITTED) == 102 and "static_assert(kDmaPairs == 102" in text
    assert "kDmaMinSlotBytes = 6912" in text and "kDmaBlocksPerCu = 2" in text and "kDmaLdsBudget = 156 * 1024" in text
    # 256 * 27 = 6912: the least slot; two workgroups' rings of 38 bits fit the budget and those of 39 do not
    assert 2 * (1024 + 4 * 2 * 256 * 38) <= 156 * 1024 < 2 * (1024 + 4 * 2 * 256 * 39)


def answer(res):
    return res.stats[0], [(a.count, a.sum_i64, a.min, a.max) for a in res.aggregations]


def cardinality(bits):
    return 2 ** bits - (3 if bits % 3 == 0 else 0)      # (still `bits` wide)


@functools.lru_cache(maxsize=None)
def filter_column(bits, n, lower_half_only=False):
    card = cardinality(bits)
    values = np.arange(card, dtype=np.int32) * 2 - 9
    if lower_half_only:      # dictIds card // 2 .. exist in the dictionary and in no doc
        col = S.Column.from_dict_ids("f", values, S.synthetic_dict_ids(900 + bits, 0, n, card // 2))
    else:
        col = S.Column.synthetic_uniform("f", n, values, seed=bits)
    assert col.bits == bits
    return col


@functools.lru_cache(maxsize=None)
def value_column(bits, n):
    """Affine values: the dictId stream is its own value plane, so the aggregated column is the `bits`-wide one."""
    col = S.Column.synthetic_uniform("v", n, (np.arange(cardinality(bits), dtype=np.int64) * 7 + 3).astype(np.int32), seed=100 + bits)
    assert col.bits == bits
    return col


@pytest.fixture
def four_ways(engine):
    def run(seg, specs, nt=None, blocks_per_cu=None, ways=("pair", "generic", "no-ring")):
        had = os.environ.get("PINOT_GPU_TEST_CUS")
        os.environ["PINOT_GPU_TEST_CUS"] = "1"      # (read when the segment opens)
        answers = []
        try:
            with engine.open(seg) as g:
                for spec in specs:
                    want = oracle.execute(seg, spec)
                    got = {}
                    for way in ways:
                        engine.reinit(**dict(WAYS[way], **{NT: nt, BPC: blocks_per_cu}))
                        got[way] = g.execute(spec)
                        assert got[way].dominant_kernel == "scan_simple_kernel", (way, got[way].dominant_kernel)
                        H.assert_results_equal(got[way], want, True)
                    assert all(answer(got[way]) == answer(got[ways[0]]) for way in ways)
                    answers.append(answer(got[ways[0]]))
        finally:
            engine.reinit(**{name: None for name in (DMA, PAIR, NT, BPC)})
            if had is None:
                os.environ.pop("PINOT_GPU_TEST_CUS", None)
            else:
                os.environ["PINOT_GPU_TEST_CUS"] = had
        return answers
    return run


def leaf(lo, hi, **kw):
    return Q.leaf(Q.Pred.dict_range(0, lo, hi, **kw))


@pytest.mark.parametrize("fbits,vbits", ADMITTED)
def test_every_admitted_pair_with_zero_to_three_tiles_per_wave(four_ways, fbits, vbits):
    card = cardinality(fbits)
    spec = Q.QuerySpec(EVERY_FUNCTION, filter=leaf(card // 4, (3 * card) // 4))
    for tiles in (3, 6, 11):
        n = 2048 * tiles - 37 - fbits
        seg = S.SegmentData("p%d_%d_%d" % (fbits, vbits, tiles), n, [filter_column(fbits, n), value_column(vbits, n)])
        four_ways(seg, [spec], blocks_per_cu=1)


def edge_specs(fbits):
    """On a filter column whose docs hold only the lower half of the dictionary."""
    card = cardinality(fbits)
    half = card // 2
    return [Q.QuerySpec([(Q.SUM, 1)], filter=leaf(0, half // 10 + 1)),                          # lo == 0, the sum alone: the headline's path
            Q.QuerySpec(EVERY_FUNCTION, filter=leaf(half // 3, half // 2 + 1)),                  # lo > 0, every function
            Q.QuerySpec([(Q.MIN, 1), (Q.MAX, 1)], filter=leaf(0, half // 4 + 1)),                # min / max without a sum
            Q.QuerySpec([(Q.COUNT, -1), (Q.MAX, 1)], filter=leaf(half // 5, half // 2, exclusive=True)),      # an exclusive leaf
            Q.QuerySpec([(Q.SUM, 1), (Q.COUNT, -1)], filter=leaf(0, half // 2, exclusive=True)),
            Q.QuerySpec(EVERY_FUNCTION, filter=leaf(half + 1, card - 1)),                        # matches nothing
            Q.QuerySpec(EVERY_FUNCTION, filter=leaf(0, card, exclusive=True)),                   # ... nor does this
            Q.QuerySpec(EVERY_FUNCTION, filter=leaf(0, half)),                                   # matches everything
            Q.QuerySpec([(Q.SUM, 1)], filter=leaf(half, card, exclusive=True))]                  # ... so does this


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 3 * 2048 - 1, 3 * 2048 + 1])
@pytest.mark.parametrize("fbits,vbits", EXTREMES)
def test_the_headline_and_the_extreme_pairs_at_the_tile_edges(four_ways, fbits, vbits, n):
    seg = S.SegmentData("e%d_%d_%d" % (fbits, vbits, n), n, [filter_column(fbits, n, True), value_column(vbits, n)])
    specs = edge_specs(fbits)
    assert oracle.execute(seg, specs[5]).aggregations[0].count == 0 and oracle.execute(seg, specs[7]).aggregations[0].count == n
    default = four_ways(seg, specs, nt=0, blocks_per_cu=1)
    non_temporal = four_ways(seg, specs, nt=1, blocks_per_cu=1, ways=("pair", "generic"))
    assert default == non_temporal


@pytest.mark.parametrize("fbits,vbits", EXTREMES)
def test_two_different_queries_back_to_back_on_one_open_segment(engine, fbits, vbits):
    """Nothing a launch reads from a slot is left over from the launch before."""
    n = 2048 * 21 + 1234
    seg = S.SegmentData("b%d_%d" % (fbits, vbits), n, [filter_column(fbits, n, True), value_column(vbits, n)])
    a, b = edge_specs(fbits)[:2]
    want = {id(a): oracle.execute(seg, a), id(b): oracle.execute(seg, b)}
    had = os.environ.get("PINOT_GPU_TEST_CUS")
    os.environ["PINOT_GPU_TEST_CUS"] = "1"
    try:
        with engine.open(seg) as g:
            engine.reinit(**WAYS["pair"])
            for spec in (a, b, b, a, b, a):
                H.assert_results_equal(g.execute(spec), want[id(spec)], True)
    finally:
        engine.reinit(**{name: None for name in (DMA, PAIR, NT, BPC)})
        if had is None:
            os.environ.pop("PINOT_GPU_TEST_CUS", None)
        else:
            os.environ["PINOT_GPU_TEST_CUS"] = had


@pytest.mark.parametrize("fbits,vbits", [(6, 20), (19, 20)])
def test_pairs_just_outside_the_rule_answer_through_the_generic_kernel(four_ways, fbits, vbits):
    """26 and 39 bits: no instance; with the switch at 2 the ring kernel's generic form takes them."""
    assert (fbits, vbits) not in ADMITTED
    n = 2048 * 9 + 555
    seg = S.SegmentData("o%d_%d" % (fbits, vbits), n, [filter_column(fbits, n, True), value_column(vbits, n)])
    four_ways(seg, edge_specs(fbits))
