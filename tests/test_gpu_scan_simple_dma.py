"""GPU tests of scan_simple_dma_kernel (pinot_amd/csrc/pg_scan_simple_dma.h): the pipelined kernel's queries -- one dictionary-range leaf
AND one aggregated packed column -- with the two columns streamed through a wave-private ring of S = 2 LDS slots by LDS-DMA loads, S - 1
tiles ahead of the decode.  Every case runs three ways -- PINOT_GPU_SCAN_SIMPLE_DMA=2 (the ring kernel whenever the shape allows), =0
(scan_simple_pipe_kernel / scan_simple_kernel, by their rule) and the oracle -- and all three are bit equal; every kernel reports
`scan_simple_kernel`.

The shapes are the smallest at which a ring can go wrong: waves with 0, 1, S - 2, S - 1, S, S + 1 and 2 S + 1 tiles (a prologue that
fills fewer than S - 1 slots, a loop that never runs, a drain of every length), every width as the filter and as the aggregated column
(every remainder of a chunk's last 1 KiB instruction, every alignment of a lane's dwords in the slot), segments that end on a tile
boundary, the masks at their edges, both cache policies, and two different queries back to back on one open segment."""
import os

import numpy as np
import pytest

from oracle import oracle
from pinot_amd import query as Q
from pinot_amd import segment as S
import helpers as H

pytestmark = pytest.mark.gpu

ALL_FUNCTIONS = [(Q.COUNT, -1), (Q.MIN, 1), (Q.MAX, 1), (Q.AVG, 1)]
RING_SWITCHES = ("PINOT_GPU_SCAN_SIMPLE_DMA", "PINOT_GPU_SCAN_SIMPLE_DMA_NT", "PINOT_GPU_SCAN_SIMPLE_DMA_BLOCKS_PER_CU")


def answer(res):
    return res.stats[0], [(a.count, a.sum_i64, a.min, a.max) for a in res.aggregations]


@pytest.fixture
def three_ways(engine):
    def run(seg, specs, cus=None, nt=None, blocks_per_cu=None):
        """Every spec on one open segment: the ring kernel, the kernels without it, the oracle.  cus: PINOT_GPU_TEST_CUS (read when the
        segment opens); nt / blocks_per_cu: the ring's switches (None: the rule's choice)."""
        had = os.environ.get("PINOT_GPU_TEST_CUS")
        if cus is not None:
            os.environ["PINOT_GPU_TEST_CUS"] = str(cus)
        answers = []
        try:
            with engine.open(seg) as g:
                for spec in specs:
                    want = oracle.execute(seg, spec)
                    got = {}
                    for mode in ("2", "0"):
                        engine.reinit(PINOT_GPU_SCAN_SIMPLE_DMA=mode, PINOT_GPU_SCAN_SIMPLE_DMA_NT=nt,
                                      PINOT_GPU_SCAN_SIMPLE_DMA_BLOCKS_PER_CU=blocks_per_cu)
                        got[mode] = g.execute(spec)
                        assert got[mode].dominant_kernel == "scan_simple_kernel", (mode, got[mode].dominant_kernel)
                        H.assert_results_equal(got[mode], want, True)
                    assert answer(got["2"]) == answer(got["0"])
                    answers.append(answer(got["2"]))
        finally:
            engine.reinit(**{name: None for name in RING_SWITCHES})
            if cus is not None:
                if had is None:
                    os.environ.pop("PINOT_GPU_TEST_CUS", None)
                else:
                    os.environ["PINOT_GPU_TEST_CUS"] = had
        return answers
    return run


def headline_columns(n, seed):
    """f: 10 bits (1000 values), v: 17 bits (100 000 values, affine: the dictId stream is its own value plane) -- the headline's widths."""
    f = S.Column.synthetic_uniform("f", n, np.arange(1000, dtype=np.int32), seed=seed)
    v = S.Column.synthetic_uniform("v", n, (np.arange(100000, dtype=np.int64) * 7 + 3).astype(np.int32), seed=seed + 1)
    assert f.bits == 10 and v.bits == 17
    return f, v


def headline_specs():
    return [Q.QuerySpec([(Q.SUM, 1)], filter=Q.leaf(Q.Pred.dict_range(0, 0, 100))),
            Q.QuerySpec(ALL_FUNCTIONS, filter=Q.leaf(Q.Pred.dict_range(0, 300, 800)))]


@pytest.mark.parametrize("tiles", [1, 2, 3, 4, 7, 8, 11, 12, 15, 16, 19, 20, 23, 24, 28, 31])
def test_tiles_per_wave_on_one_compute_unit(three_ways, tiles):
    """One CU and one workgroup of four waves (PINOT_GPU_SCAN_SIMPLE_DMA_BLOCKS_PER_CU=1): wave w owns tiles w, w + 4, ...  1 to 3 tiles
    leave waves without one (S - 2 = 0 tiles); 4 k tiles give every wave k = 1 .. 7 (S - 1 = 1, S = 2, S + 1 = 3, 2 S + 1 = 5 and beyond);
    4 k + 3 tiles give three waves k + 1 and one k: a workgroup whose waves drain at different lengths.  Ragged
    last tiles."""
    n = 2048 * tiles - 37
    f, v = headline_columns(n, 10 + tiles)
    three_ways(S.SegmentData("t%d" % tiles, n, [f, v]), headline_specs(), cus=1, blocks_per_cu=1)


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049])
def test_doc_counts_around_one_tile(three_ways, n):
    f, v = headline_columns(n, 70 + n % 13)
    three_ways(S.SegmentData("n%d" % n, n, [f, v]), headline_specs(), cus=1)


def test_two_workgroups_on_one_compute_unit(three_ways):
    """The rule's grid on one CU (two workgroups): 100 003 docs = 49 tiles for eight waves."""
    f, v = headline_columns(100003, 8)
    three_ways(S.SegmentData("two", 100003, [f, v]), headline_specs(), cus=1)


def test_most_waves_without_a_tile_on_the_full_grid(three_ways):
    f, v = headline_columns(70001, 5)
    three_ways(S.SegmentData("full", 70001, [f, v]), headline_specs())


def width_case(three_ways, fbits, vbits):
    n = 6151 + 37 * fbits + 2048 * 9
    cf = 2 ** fbits - (1 if fbits > 1 and fbits % 3 == 0 else 0)
    cv = 2 ** vbits - (1 if vbits > 1 and vbits % 2 == 0 else 0)
    f = S.Column.synthetic_uniform("f", n, np.arange(cf, dtype=np.int32) * 2 - 9, seed=fbits)
    v = S.Column.synthetic_uniform("v", n, (np.arange(cv, dtype=np.int64) * 7 + 3).astype(np.int32), seed=100 + vbits)
    assert f.bits == fbits and v.bits == vbits
    lo, hi = cf // 4, max(cf // 4 + 1, (3 * cf) // 4)
    three_ways(S.SegmentData("w%d_%d" % (fbits, vbits), n, [f, v]),
               [Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, 1), (Q.MIN, 1), (Q.MAX, 1), (Q.AVG, 1)], filter=Q.leaf(Q.Pred.dict_range(0, lo, hi))),
                Q.QuerySpec([(Q.SUM, 1)], filter=Q.leaf(Q.Pred.dict_range(0, 0, max(1, cf // 3)))),
                Q.QuerySpec([(Q.COUNT, -1), (Q.MAX, 1)], filter=Q.leaf(Q.Pred.dict_range(0, lo, hi, exclusive=True)))], cus=1)


@pytest.mark.parametrize("fbits", range(1, 21))
def test_every_filter_width_with_a_17_bit_value_column(three_ways, fbits):
    """Every remainder of 256 * bits mod 1024 in the filter chunk's last instruction, every alignment of the value chunk behind it in the slot
    and of a lane's dwords; three or four tiles per wave of one CU's eight."""
    width_case(three_ways, fbits, 17)


@pytest.mark.parametrize("vbits", range(1, 21))
def test_every_value_width_with_a_10_bit_filter(three_ways, vbits):
    width_case(three_ways, 10, vbits)


@pytest.mark.parametrize("fbits,vbits", [(1, 1), (20, 20), (13, 17), (17, 9), (17, 16), (20, 17)])
def test_the_smallest_and_largest_slots_and_the_pairs_the_pipelined_kernel_lacks(three_ways, fbits, vbits):
    """(1, 1): slots of 512 bytes, one instruction of 16 lanes per chunk.  (20, 20): 10 240 bytes, ten instructions per tile.  <4, 5>, <5, 3>,
    <5, 4> and <5, 5> of scan_simple_pipe_kernel do not exist (registers): (13, 17), (17, 9), (17, 16) and (20, 17) are such pairs."""
    width_case(three_ways, fbits, vbits)


@pytest.mark.parametrize("tiles", [1, 2, 21, 45])
def test_segments_that_end_on_a_tile_boundary(three_ways, tiles):
    n = 2048 * tiles
    f, v = headline_columns(n, 40 + tiles)
    three_ways(S.SegmentData("b%d" % tiles, n, [f, v]), headline_specs(), cus=1)


def test_masks_at_their_edges(three_ways):
    n = 11 * 2048 + 777
    rng = np.random.default_rng(11)
    ids = rng.integers(0, 500, n).astype(np.int32)             # dictIds 500 .. 999 exist in the dictionary and in no doc ...
    ids[n - 1] = 777                                           # ... but for the last doc of the last tile
    f = S.Column.from_dict_ids("f", np.arange(1000, dtype=np.int32) * 3 - 50, ids)
    v = S.Column.synthetic_uniform("v", n, (np.arange(100000, dtype=np.int64) * 7 + 3).astype(np.int32), seed=3)
    seg = S.SegmentData("masks", n, [f, v])
    leaf = lambda lo, hi, **kw: Q.leaf(Q.Pred.dict_range(0, lo, hi, **kw))
    specs = []
    for aggs in ([(Q.SUM, 1)], ALL_FUNCTIONS):
        specs += [Q.QuerySpec(aggs, filter=leaf(600, 700)),                    # no doc matches
                  Q.QuerySpec(aggs, filter=leaf(0, 999)),                      # every doc matches
                  Q.QuerySpec(aggs, filter=leaf(777, 778)),                    # one match: the last doc of the last tile
                  Q.QuerySpec(aggs, filter=leaf(123, 345)),                    # lo != 0
                  Q.QuerySpec(aggs, filter=leaf(100, 400, exclusive=True)),    # an exclusive range
                  Q.QuerySpec(aggs, filter=leaf(0, 778, exclusive=True))]      # ... that excludes every doc
    three_ways(seg, specs, cus=1, blocks_per_cu=1)
    with_match = oracle.execute(seg, specs[2])
    assert with_match.aggregations[0].count == 1


def test_both_cache_policies_give_one_answer(three_ways):
    n = 2048 * 61 + 5
    f, v = headline_columns(n, 21)
    seg = S.SegmentData("policy", n, [f, v])
    default = three_ways(seg, headline_specs(), cus=1, nt=0)
    non_temporal = three_ways(seg, headline_specs(), cus=1, nt=1)
    assert default == non_temporal


def test_two_different_queries_back_to_back_on_one_open_segment(engine):
    """Nothing a launch reads from a slot is left over from the launch before: the same segment, the ring kernel, two queries that differ in
    range and functions, alternated; each answer is the oracle's every time."""
    n = 2048 * 37 + 1234
    f, v = headline_columns(n, 31)
    seg = S.SegmentData("pair", n, [f, v])
    a, b = headline_specs()
    want = {id(a): oracle.execute(seg, a), id(b): oracle.execute(seg, b)}
    had = os.environ.get("PINOT_GPU_TEST_CUS")
    os.environ["PINOT_GPU_TEST_CUS"] = "1"
    try:
        with engine.open(seg) as g:
            engine.reinit(PINOT_GPU_SCAN_SIMPLE_DMA="2")
            for spec in (a, b, b, a, b, a):
                H.assert_results_equal(g.execute(spec), want[id(spec)], True)
    finally:
        engine.reinit(**{name: None for name in RING_SWITCHES})
        if had is None:
            os.environ.pop("PINOT_GPU_TEST_CUS", None)
        else:
            os.environ["PINOT_GPU_TEST_CUS"] = had
