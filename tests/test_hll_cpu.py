"""CPU tests of DISTINCTCOUNTHLL: the numpy model of tests/hll_cases.py is pinned to the reference's own numbers
(InterSegmentAggregationSingleValueQueriesTest.testDistinctCountHLL :261-284, over the committed fixture), the C header and its Python mirror
agree on the additions, the host mirror parses the function, merges registers by the maximum through host.combine_hll, gives the estimate as
the LONG final result and orders by it.  Everything is integers: no tolerance anywhere."""
import math
import os
import re

import numpy as np
import pytest

import distinct_cases as D
import helpers as H
import hll_cases as HL
from pinot_amd import _abi
from pinot_amd import host
from pinot_amd import query as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    seg = H.golden_segment()
    return seg, {(f, g): HL.model(seg, HL.golden_spec(seg, f, g)) for _, f, g in HL.GOLDEN_CASES}


# ---- the model against the reference's eight numbers ----
@pytest.mark.parametrize("row,filtered,grouped", HL.GOLDEN_CASES)
def test_the_model_reproduces_the_reference_rows(golden, row, filtered, grouped):
    seg, models = golden
    want = HL.GOLDEN_ROWS[row]
    spec = HL.golden_spec(seg, filtered, grouped)
    sets = models[(filtered, grouped)]
    assert int(D.matching_docs(seg, spec).sum()) == want["stats"][0]
    if not grouped:
        assert HL.golden_pair(sets) == (want["v1"], want["v2"])
        # four copies of the segment merge to the same registers
        for a in (0, 1):
            merged = sets[a]
            for _ in range(3):
                merged = HL.merge(merged, sets[a])
            assert np.array_equal(merged, sets[a])
        return
    top = max(sets, key=lambda g: HL.golden_pair(sets[g]))                # ORDER BY v1 DESC, v2 DESC LIMIT 1
    assert top == D.golden_group_id(seg)
    assert HL.golden_pair(sets[top]) == (want["v1"], want["v2"])


def test_the_host_estimator_is_the_models(golden):
    _, models = golden
    for sets in (models[(False, False)], models[(True, False)]):
        for regs in sets.values():
            assert host.hll_cardinality(regs) == HL.cardinality(regs)
    rng = np.random.default_rng(2)
    for log2m in range(4, 15):
        m = 1 << log2m
        for fill in (0.0, 0.03, 0.5, 1.0):
            regs = (rng.integers(1, 33 - log2m + 1, m) * (rng.random(m) < fill)).astype(np.uint8)
            assert host.hll_cardinality(regs) == HL.cardinality(regs), (log2m, fill)
    assert host.hll_cardinality(np.zeros(256, np.uint8)) == 0
    with pytest.raises(ValueError):
        host.hll_cardinality(np.zeros(100, np.uint8))


def test_the_four_types_hash_the_long_the_specification_names():
    # INT: sign-extended; LONG: itself; FLOAT: the 32 stored bits sign-extended (NOT the float widened to a double); DOUBLE: its 64 bits
    assert HL.longs_of([-1], np.int32)[0] == -1 and HL.longs_of([2 ** 31 - 1], np.int32)[0] == 2 ** 31 - 1
    assert HL.longs_of([-2 ** 63], np.int64)[0] == -2 ** 63
    f = np.array([0x80000000, 0, 0x7FC00001, 0x3F800000], dtype=np.uint32).view(np.float32)
    assert list(HL.longs_of(f, np.float32)) == [-2 ** 31, 0, 0x7FC00001, 0x3F800000]
    d = np.array([0x8000000000000000, 0, 0x7FF8000000000001], dtype=np.uint64).view(np.float64)
    assert list(HL.longs_of(d, np.float64)) == [-2 ** 63, 0, 0x7FF8000000000001]
    # -0.0 and 0.0 are two values, two NaN payloads are two values; a float and the same number as a double are not one value
    assert len(set(HL.hash_long(HL.longs_of(f, np.float32)).tolist())) == 4
    assert HL.hash_long(HL.longs_of([1.0], np.float32))[0] != HL.hash_long(HL.longs_of([1.0], np.float64))[0]
    # the hash itself, worked by hand in Python integers for one long with a non-zero high word
    def by_hand(v):
        M, mask = 0x5BD1E995, 0xFFFFFFFF
        v &= (1 << 64) - 1
        k = ((v & mask) * M) & mask; k ^= k >> 24; h = (k * M) & mask
        k = ((v >> 32) * M) & mask; k ^= k >> 24; h = (h * M) & mask; h ^= (k * M) & mask
        h ^= h >> 13; h = (h * M) & mask; h ^= h >> 15
        return h
    for v in (0, 1, -1, 2 ** 40 + 12345, -2 ** 63, 296467636):
        assert int(HL.hash_long(np.array([v], dtype=np.int64))[0]) == by_hand(v), v
    # rank: at most 32 - log2m + 1, from the sentinel bit
    for log2m in (4, 8, 14):
        regs = HL.registers_of_longs(np.arange(200000, dtype=np.int64), log2m)
        assert regs.max() <= 32 - log2m + 1 and regs.min() >= 1


def test_the_header_the_kernels_include_gives_the_models_registers():
    """pinot_amd/csrc/pg_hll.h (hash, index, rank -- what host and device code share) through the host mirror, against the numpy model: longs of
    every shape of high word, every log2m; and the narrowing of a widened FLOAT dictionary entry, NaN payloads included."""
    rng = np.random.default_rng(4)
    longs = np.concatenate([rng.integers(-2 ** 63, 2 ** 63 - 1, 50000), rng.integers(-2 ** 31, 2 ** 31, 50000), np.arange(-5, 5),
                            np.array([2 ** 63 - 1, -2 ** 63, 2 ** 32, -2 ** 32 - 1, 296467636])]).astype(np.int64)
    for log2m in range(4, 15):
        assert np.array_equal(host.hll_offer_longs(longs, log2m), HL.registers_of_longs(longs, log2m)), log2m
    assert not np.any(host.hll_offer_longs(np.zeros(0, np.int64), 8))
    for log2m in (3, 15):
        with pytest.raises(ValueError):
            host.hll_offer_longs(longs[:4], log2m)
    floats = np.concatenate([(rng.standard_normal(2000) * 1e3).astype(np.float32),
                             np.array([0x80000000, 0, 0x7FC00001, 0x7FC12345, 0xFFC00000, 0x7F800000, 0xFF800000, 0x00000001, 0x7F7FFFFF], dtype=np.uint32).view(np.float32)])
    widened = floats.astype(np.float64).view(np.uint64)                 # (numpy widens as the engine does: exactly, quiet NaN payloads kept)
    back = np.array([host.hll_float_bits_of_widened(int(b)) for b in widened], dtype=np.uint32)
    assert np.array_equal(back, floats.view(np.uint32))


def test_a_rank_the_sketch_cannot_hold_is_refused():
    regs = np.zeros(256, np.uint8)
    regs[7] = 25                                                        # log2m 8: a rank is at most 25
    assert host.hll_cardinality(regs) == HL.cardinality(regs)
    regs[7] = 26
    with pytest.raises(ValueError):
        host.hll_cardinality(regs)
    regs[7] = 200                                                       # (would shift past a 64-bit word in the estimator)
    with pytest.raises(ValueError):
        host.hll_cardinality(regs)
    with pytest.raises(host.HostError) as e:
        host.combine_hll("SELECT DISTINCTCOUNTHLL(m) FROM t", [[((), [_cell(regs)])]])
    assert "register of rank 200" in str(e.value)


# ---- the header and its mirrors ----
def test_the_header_and_its_mirror_agree_on_the_additions():
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert re.search(r"#define\s+PG_ABI_VERSION\s+5\b", header) and _abi.PG_ABI_VERSION == 5
    assert re.search(r"\bPG_AGG_DISTINCTCOUNTHLL\s*=\s*7\b", header) and _abi.PG_AGG_DISTINCTCOUNTHLL == 7 == Q.DISTINCTCOUNTHLL
    assert re.search(r"#define\s+PG_AGG_HLL\(log2m\)\s+\(PG_AGG_DISTINCTCOUNTHLL \| \(\(log2m\) << 8\)\)", header)
    assert _abi.PG_AGG_HLL(12) == 7 | (12 << 8) == Q.hll(12) and Q.hll() == 7 | (8 << 8)
    assert Q.is_hll(Q.hll(4)) and Q.is_hll(7) and not Q.is_hll(Q.DISTINCTCOUNT) and Q.hll_log2m(7) == 8 and Q.hll_log2m(Q.hll(14)) == 14
    for name, value in (("PG_HLL_MIN_LOG2M", 4), ("PG_HLL_MAX_LOG2M", 14), ("PG_HLL_DEFAULT_LOG2M", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header) and getattr(_abi, name) == value
    assert re.search(r"#define\s+PG_HLL_GROUP_MAX_BYTES\s+\(1ull << 30\)", header) and _abi.PG_HLL_GROUP_MAX_BYTES == 1 << 30
    assert re.search(r"\bPG_KERNEL_SCAN_HLL\s*=\s*20\b", header) and _abi.KERNEL_NAMES[20] == "scan_hll_kernel"
    assert re.search(r"\bPG_KERNEL_GROUP_HLL\s*=\s*21\b", header) and _abi.KERNEL_NAMES[21] == "group_hll_kernel"
    assert "pg_result_hll_registers" in header and any(name == "pg_result_hll_registers" for name, _, _ in _abi.ABI_SYMBOLS)
    # the one header host and device code share states the same constants
    shared = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_hll.h")).read()
    assert re.search(r"kHllMinLog2m = 4, kHllMaxLog2m = 14, kHllDefaultLog2m = 8", shared) and re.search(r"kHllFunction = 7\b", shared)
    assert "0x5bd1e995" in shared


# ---- the parser ----
def test_the_host_mirror_parses_the_spellings():
    q = host.parse_sql("SELECT DISTINCTCOUNTHLL(column1) AS v1, DISTINCT_COUNT_HLL(column3), distinctcount_hll(column1, 12) FROM testTable WHERE column1 > 100000000")
    assert q["aggregations"] == ["distinctcounthll(column1)", "distinctcounthll(column3)", "distinctcounthll(column1)"] and q["hasFilter"]
    q = host.parse_sql("SELECT DISTINCTCOUNTHLL(column1) AS v1, DISTINCTCOUNTHLL(column3) AS v2 FROM testTable GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1")
    assert q["groupBy"] == ["column9"] and q["limit"] == 1
    assert [(o["expression"], o["asc"]) for o in q["orderBy"]] == [("distinctcounthll(column1)", False), ("distinctcounthll(column3)", False)]
    q = host.parse_sql("SELECT COUNT(*), DistinctCountHLL(column1) FROM testTable GROUP BY column9 ORDER BY distinct_count_hll(column1) DESC")
    assert q["aggregations"] == ["count(*)", "distinctcounthll(column1)"] and q["orderBy"][0]["expression"] == "distinctcounthll(column1)"
    for log2m in (4, 14, "'9'"):
        host.parse_sql("SELECT DISTINCTCOUNTHLL(column1, %s) FROM testTable" % log2m)


@pytest.mark.parametrize("log2m", ["3", "15", "0", "-1", "100"])
def test_a_log2m_outside_the_range_is_rejected(log2m):
    with pytest.raises(host.HostError) as e:
        host.parse_sql("SELECT DISTINCTCOUNTHLL(column1, %s) FROM testTable" % log2m)
    assert e.value.status in (1, 2)
    assert re.search(r"log2m %s is not offloaded \(4 to 14 are\)|Invalid log2m: -" % re.escape(log2m), str(e.value)), str(e.value)


def test_other_hll_functions_and_malformed_arguments_are_rejected():
    for sql, message in (("SELECT DISTINCTCOUNTRAWHLL(column1) FROM testTable", r"DISTINCTCOUNTHLL/PERCENTILE are offloaded, got DISTINCTCOUNTRAWHLL"),
                         ("SELECT DISTINCTCOUNTHLLPLUS(column1) FROM testTable", r"DISTINCTCOUNTHLL/PERCENTILE are offloaded, got DISTINCTCOUNTHLLPLUS"),
                         ("SELECT DISTINCTCOUNTHLL(*) FROM testTable", r"'\*' is only valid in COUNT\(\*\)"),
                         ("SELECT DISTINCTCOUNTHLL(column1, x) FROM testTable", r"Invalid log2m: x"),
                         ("SELECT DISTINCTCOUNTHLL(column1, 8, 9) FROM testTable", r"only identifier arguments are offloaded"),
                         ("SELECT COUNT(*) FROM testTable GROUP BY column9 ORDER BY DISTINCTCOUNTHLL(column1)", r"a DISTINCTCOUNTHLL that appears only in ORDER BY")):
        with pytest.raises(host.HostError) as e:
            host.parse_sql(sql)
        assert e.value.status in (1, 2), sql
        assert re.search(message, str(e.value)), (sql, str(e.value))


# ---- the combine, from host-supplied registers (no device) ----
def _cell(regs):
    return (0, 0.0, 0.0, 0.0, False, regs)


SQL = "SELECT DISTINCTCOUNTHLL(column1) AS v1, DISTINCTCOUNTHLL(column3) AS v2 FROM testTable"


@pytest.mark.parametrize("row,filtered,grouped", HL.GOLDEN_CASES)
def test_the_combine_of_four_segments_returns_the_reference_rows(golden, row, filtered, grouped):
    seg, models = golden
    want = HL.GOLDEN_ROWS[row]
    sets = models[(filtered, grouped)]
    if not grouped:
        blocks = [[((), [_cell(sets[0]), _cell(sets[1])])] for _ in range(4)]
        out = host.combine_hll(SQL, blocks)
        assert out["combined"]["final"] == [want["v1"], want["v2"]]
        assert [v["registers"] for v in out["combined"]["intermediate"]] == [sets[0].tolist(), sets[1].tolist()]
        return
    c9 = seg.columns[seg.column_index("column9")]
    block = [((c9.value_of(gid),), [_cell(regs[0]), _cell(regs[1])]) for gid, regs in sorted(sets.items())]
    out = host.combine_hll(SQL + " GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1", [block] * 4, [host.KEY_INT])
    assert out["resultTable"]["rows"] == [[want["v1"], want["v2"]]]
    assert out["reduced"] == [[HL.GOLDEN_GROUP_KEY, want["v1"], want["v2"]]]
    assert all(isinstance(x, int) for x in out["reduced"][0])            # a LONG final result


def test_the_merge_is_the_register_wise_maximum_and_orders_by_the_estimate():
    a = HL.registers_of_longs(np.arange(0, 3000, dtype=np.int64))
    b = HL.registers_of_longs(np.arange(2000, 9000, dtype=np.int64))
    small = HL.registers_of_longs(np.arange(50, dtype=np.int64))
    sql = "SELECT DISTINCTCOUNTHLL(m) AS v FROM t GROUP BY d ORDER BY v DESC LIMIT 2"
    blocks = [[((1,), [_cell(a)]), ((2,), [_cell(small)])], [((1,), [_cell(b)]), ((3,), [_cell(b)])]]
    out = host.combine_hll(sql, blocks, [host.KEY_INT])
    groups = {tuple(g["key"]): g for g in out["combined"]["groups"]}
    assert groups[(1,)]["intermediate"][0]["registers"] == np.maximum(a, b).tolist()
    assert groups[(1,)]["final"] == [HL.cardinality(np.maximum(a, b))] == [HL.cardinality(HL.registers_of_longs(np.arange(9000, dtype=np.int64)))]
    assert out["reduced"] == [[1, HL.cardinality(np.maximum(a, b))], [3, HL.cardinality(b)]]


def test_the_size_rule_of_merge():
    """DistinctCountHLLAggregationFunction.merge :333-350: sketches of different sizes -- the one whose cardinality is 0 gives way; two non-empty
    ones cannot be merged."""
    r8 = HL.registers_of_longs(np.arange(1000, dtype=np.int64), 8)
    r12 = HL.registers_of_longs(np.arange(1000, dtype=np.int64), 12)
    sql = "SELECT DISTINCTCOUNTHLL(m, 12) FROM t"
    out = host.combine_hll(sql, [[((), [_cell(np.zeros(256, np.uint8))])], [((), [_cell(r12)])]])
    assert out["combined"]["intermediate"][0]["registers"] == r12.tolist()
    out = host.combine_hll(sql, [[((), [_cell(r12)])], [((), [_cell(np.zeros(256, np.uint8))])]])
    assert out["combined"]["intermediate"][0]["registers"] == r12.tolist()
    out = host.combine_hll(sql, [[((), [_cell(r12)])], [((), [_cell([])])]])              # an empty cell: an empty sketch of the function's log2m
    assert out["combined"]["final"] == [HL.cardinality(r12)]
    with pytest.raises(host.HostError) as e:
        host.combine_hll(sql, [[((), [_cell(r8)])], [((), [_cell(r12)])]])
    assert "different sizes" in str(e.value)


def test_rounding_is_floor_of_x_plus_a_half():
    """Math.round is floor(x + 0.5); banker's rounding (Python's round, numpy's rint) differs exactly where the estimate ends in .5.  In the
    linear-counting branch the estimate is m ln(m / zeros), which is never a half integer for 0 < zeros < m (ln of a rational other than 1 is
    irrational); in the default branch it is alphaMM / sum with sum a dyadic rational.  No register set whose estimate ends in .5 was found: the
    search here is 300 random register sets of log2m 4 (ranks 0 to 29 drawn uniformly; the draws that land in the linear-counting branch are
    counted and left out), and the closest any default-branch estimate comes to a half integer stays above 1e-9.  So no constructed register set
    separates the two roundings; what is pinned instead is that the two roundings differ on a half, and that the host's estimator equals
    floor(x + 0.5) of the default-branch estimate on every searched set."""
    assert math.floor(2.5 + 0.5) == 3 and round(2.5) == 2                 # the two roundings do differ on a half
    m, log2m = 16, 4
    closest = 1.0
    searched = linear = 0
    rng = np.random.default_rng(9)
    for _ in range(300):
        regs = rng.integers(0, 30, m).astype(np.uint8)
        total = float(np.sum(1.0 / (np.uint64(1) << regs.astype(np.uint64)).astype(np.float64)))
        estimate = 0.673 * m * m / total
        linear += estimate <= 2.5 * m
        if estimate > 2.5 * m:
            searched += 1
            closest = min(closest, abs(estimate - math.floor(estimate) - 0.5))
            assert host.hll_cardinality(regs) == int(math.floor(estimate + 0.5)) == HL.cardinality(regs)
    assert closest > 1e-9 and searched + linear == 300 and searched >= 200, (closest, searched, linear)


# ---- the constructed register corpus: values whose hash is chosen (hll_cases.long_with_hash) ----
def test_the_hash_is_inverted_for_every_high_word():
    rng = np.random.default_rng(31)
    hashes = [int(x) for x in rng.integers(0, 2 ** 32, 1000)] + [0, 1, 2 ** 32 - 1, 2 ** 31]
    hashes += [HL.hash_of_target(log2m, j, r) for log2m in HL.CORPUS_LOG2M for j, r in HL.corpus_targets(log2m)]
    his = [int(x) for x in rng.integers(0, 2 ** 32, len(hashes))]
    his[:4] = [0, 0xFFFFFFFF, 0x80000000, 1]
    longs = np.array([HL.long_with_hash(x, hi) for x, hi in zip(hashes, his)], dtype=np.int64)
    assert np.array_equal((longs.view(np.uint64) >> np.uint64(32)).astype(np.int64), np.array(his, dtype=np.int64))
    assert np.array_equal(HL.hash_long(longs).astype(np.int64), np.array(hashes, dtype=np.int64))
    # through the header the kernels include: one long at a time, the register and the rank its hash was built for
    for log2m in HL.CORPUS_LOG2M:
        for j, r in HL.corpus_targets(log2m):
            for hi in (0, 0xFFFFFFFF, 0x12345678):
                one = np.array([HL.long_with_hash(HL.hash_of_target(log2m, j, r), hi)], dtype=np.int64)
                regs = host.hll_offer_longs(one, log2m)
                assert regs[j] == r and np.count_nonzero(regs) == 1, (log2m, j, r, hi)
                assert np.array_equal(regs, HL.registers_of_longs(one, log2m))
    # ints: the candidate whose sign agrees with its high word, or none
    found = 0
    for x in hashes:
        v = HL.int_with_hash(x)
        if v is not None:
            found += 1
            assert -2 ** 31 <= v < 2 ** 31 and int(HL.hash_long(np.array([v], dtype=np.int64))[0]) == x
            assert int(HL.hash_long(HL.longs_of(np.array([v], dtype=np.int32), np.int32))[0]) == x
        else:
            assert all(not -2 ** 31 <= HL.long_with_hash(x, hi) < 2 ** 31 for hi in (0, -1))
    assert found >= len(hashes) // 4                                     # (each of the two candidates agrees half the time)
    assert HL.int_with_hash(HL.hash_of_target(8, 255, 25)) is None       # index 255 at log2m 8 with the largest rank: no int hashes there


def test_the_corpus_reaches_its_targets():
    """Every target (index 0 / a middle index / the last index) x (rank 1, 2, max - 1, max) at log2m 4, 8, 14: LONG and DOUBLE reach each
    one exactly; INT and FLOAT the nearest index a 32-bit value can reach, with the rank wanted."""
    wide, narrow = HL.corpus_values(64), HL.corpus_values(32)
    for log2m in HL.CORPUS_LOG2M:
        m, top = 1 << log2m, 32 - log2m + 1
        assert {(j, r) for (l, j, r) in wide if l == log2m} == set(HL.corpus_targets(log2m))
        assert (log2m, 0, top) in wide and (log2m, m - 1, top) in wide    # the first and the last register hold the largest rank
        assert sorted(r for (l, j, r) in narrow if l == log2m) == sorted(r for _, r in HL.corpus_targets(log2m))
        for table, dtype in ((wide, np.int64), (narrow, np.int32)):
            for (l, j, r), v in table.items():
                if l != log2m:
                    continue
                regs = HL.registers(np.array([v], dtype=dtype), dtype, log2m)
                assert regs[j] == r and np.count_nonzero(regs) == 1, (log2m, j, r, v)
                assert np.array_equal(host.hll_offer_longs(HL.longs_of(np.array([v], dtype=dtype), dtype), log2m), regs)


@pytest.mark.parametrize("num_docs", HL.CORPUS_SIZES)
def test_the_corpus_orders_the_largest_rank_before_and_after_the_smaller_ones(num_docs):
    wide = HL.corpus_values(64)
    targets = list(wide)
    order = HL.corpus_order(num_docs, targets)
    assert order.shape == (num_docs,)
    ranks = {}
    for i, (log2m, j, r) in enumerate(targets):
        ranks.setdefault((log2m, j), {})[i] = r
    for register, entries in ranks.items():
        big = max(entries, key=entries.get)
        at_big = np.flatnonzero(order == big)
        for i in entries:
            if i != big:
                at = np.flatnonzero(order == i)
                assert at.size and at_big.min() < at.min() and at_big.max() > at.max(), (register, entries[i])
    # three runs of 64 consecutive docs of a largest-rank value: at doc 0, inside a tile, ending in the last doc
    is_big = lambda i: targets[i][2] == 32 - targets[i][0] + 1
    for first in (0, (2048 + 1024 if num_docs > 4096 else num_docs // 2) - 32, num_docs - 64):
        run = order[first: first + 64]
        assert len(set(run.tolist())) == 1 and is_big(int(run[0])), first
    if num_docs >= 3 * 2048:
        tile = order[2 * 2048: 3 * 2048 - 64].reshape(-1, 32)
        assert np.all(tile == tile[0])                                   # the same position of every lane offers the same register


# ---- the fold segments of tests/test_gpu_hll_edges.py ----
def test_the_fold_segments_set_the_edges_of_every_chunk():
    """launch_hll_fold's arithmetic restated: 256 words per workgroup, at most 64 workgroups per row, then the words per chunk by ceiling
    division.  8192 dictIds are one chunk, 8193 two; above 524288 dictIds the cap of 64 makes chunks of more than 256 words."""
    assert [len(HL.fold_chunks(c)) for c in HL.FOLD_CARDINALITIES] == [1, 1, 2, 2, 3, 64, 64]
    assert HL.fold_chunks(524288)[0] == (0, 256) and HL.fold_chunks(524289)[0] == (0, 257) and HL.fold_chunks(524289)[-1] == (63 * 257, 16385)
    for card in HL.FOLD_CARDINALITIES:
        ids, chunk_of = HL.fold_dict_ids(card)
        chunks = HL.fold_chunks(card)
        assert chunks[0][0] == 0 and chunks[-1][1] == (card + 31) // 32 and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        for c, (first, end) in enumerate(chunks):
            assert first * 32 in ids and min(card, end * 32) - 1 in ids
        assert ids[-1] == card - 1 and len(ids) <= HL.FOLD_DOCS
