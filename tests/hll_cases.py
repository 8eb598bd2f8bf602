"""The numpy model of DISTINCTCOUNTHLL and the shared builders of its tests (tests/test_hll_cpu.py, tests/test_gpu_hll.py,
tools/kernel_coverage.py, tools/bench_variants.py).

The model restates DESIGN.md section 4.1s independently of pinot_amd/csrc/pg_hll.h: the 32-bit Murmur2 of the value as a long, the index /
rank rule of a 2^log2m register set, the estimator, the register-wise max as merge.  Registers are compared byte for byte with the engine's
over the docs `oracle.filter_bitmap` matches; nothing here has a tolerance.
"""
import math

import numpy as np

from oracle import oracle
from pinot_amd import query as Q

import distinct_cases as D

# InterSegmentAggregationSingleValueQueriesTest.testDistinctCountHLL (:261-284) over tests/golden/test_data_sv.npz: v1 = DISTINCTCOUNTHLL(column1),
# v2 = DISTINCTCOUNTHLL(column3), four copies of the segment; per-segment statistics as testDistinctCount's.
GOLDEN_GROUP_KEY = D.GOLDEN_GROUP_KEY
GOLDEN_ROWS = {
    "plain": {"v1": 5977, "v2": 23825, "stats": (30000, 0, 0, 30000)},
    "filter": {"v1": 1886, "v2": 4492, "stats": (6129, 63064, 12258, 30000)},
    "group": {"v1": 3592, "v2": 11889, "stats": (30000, 0, 90000, 30000)},
    "filter+group": {"v1": 1324, "v2": 3197, "stats": (6129, 63064, 18387, 30000)},
}
GOLDEN_CASES = [("plain", False, False), ("filter", True, False), ("group", False, True), ("filter+group", True, True)]
DEFAULT_LOG2M = 8
M = np.uint32(0x5BD1E995)


def hash_long(longs):
    """MurmurHash.hashLong over an int64 / uint64 array, in wrapping 32-bit arithmetic."""
    data = np.asarray(longs).astype(np.int64).view(np.uint64)
    with np.errstate(over="ignore"):
        k = (data & np.uint64(0xFFFFFFFF)).astype(np.uint32) * M
        k ^= k >> np.uint32(24)
        h = k * M                                                   # h = 0 ^ k * M
        k = (data >> np.uint64(32)).astype(np.uint32) * M
        k ^= k >> np.uint32(24)
        h = h * M
        h ^= k * M
        h ^= h >> np.uint32(13)
        h = h * M
        h ^= h >> np.uint32(15)
    return h


def longs_of(values, dtype):
    """The long offer(Object) hashes for every value of a column of the given numpy dtype (int32 / int64 / float32 / float64)."""
    dtype = np.dtype(dtype)
    v = np.ascontiguousarray(np.asarray(values, dtype=dtype))
    if dtype == np.int32:
        return v.astype(np.int64)
    if dtype == np.int64:
        return v
    if dtype == np.float32:
        return v.view(np.int32).astype(np.int64)                    # floatToRawIntBits, sign-extended
    if dtype == np.float64:
        return v.view(np.int64)                                     # doubleToRawLongBits
    raise ValueError(dtype)


def registers_of_longs(longs, log2m=DEFAULT_LOG2M):
    """uint8[2^log2m]: the register set after offering every long."""
    regs = np.zeros(1 << log2m, dtype=np.uint8)
    x = hash_long(longs)
    if x.size == 0:
        return regs
    j = (x >> np.uint32(32 - log2m)).astype(np.int64)
    with np.errstate(over="ignore"):
        w = (x << np.uint32(log2m)) | np.uint32((1 << (log2m - 1)) + 1)
    # numberOfLeadingZeros(w) + 1 = 32 - bit_length(w) + 1; w is never zero
    bit_length = np.floor(np.log2(w.astype(np.float64))).astype(np.int64) + 1
    rank = (33 - bit_length).astype(np.uint8)
    np.maximum.at(regs, j, rank)
    return regs


def registers(values, dtype, log2m=DEFAULT_LOG2M):
    return registers_of_longs(longs_of(values, dtype), log2m)


def merge(a, b):
    assert a.shape == b.shape
    return np.maximum(a, b)


def cardinality(regs):
    """The estimate of a register set: Java's Math.round is floor(x + 0.5)."""
    m = int(regs.shape[0])
    log2m = m.bit_length() - 1
    assert 1 << log2m == m
    alpha_mm = {4: 0.673, 5: 0.697, 6: 0.709}.get(log2m, 0.7213 / (1.0 + 1.079 / m)) * m * m
    total = float(np.sum(1.0 / (np.uint64(1) << regs.astype(np.uint64)).astype(np.float64)))
    estimate = alpha_mm / total
    if estimate <= 2.5 * m:
        zeros = int(np.count_nonzero(regs == 0))
        if zeros == 0:
            return 2 ** 63 - 1
        return int(math.floor(m * math.log(m / zeros) + 0.5))
    return int(math.floor(estimate + 0.5))


def numpy_dtype_of(column):
    """The numpy dtype of a segment column's stored type (INT / LONG / FLOAT / DOUBLE)."""
    return {0: np.int32, 1: np.int64, 2: np.float32, 3: np.float64}[int(column.stored_type)]


def set_values(seg, column, values):
    """A raw column keeps no copy of its values: the builder of a segment hands them to the model here (in the column's own dtype)."""
    seg.__dict__.setdefault("_hll_values", {})[column] = np.ascontiguousarray(values, dtype=numpy_dtype_of(seg.columns[column]))


def values_of(seg, column):
    """Every doc's value of a column AS STORED (the dictionary entry of its dictId, or the raw value given to set_values), in the column's own dtype."""
    c = seg.columns[column]
    cache = seg.__dict__.setdefault("_hll_values", {})
    if column not in cache:
        assert c.dictionary is not None, "raw column %s: set_values first" % c.name
        cache[column] = np.ascontiguousarray(np.asarray(c.dict_values)[D.dict_ids_of(seg, column)]).astype(numpy_dtype_of(c), copy=False)
    return cache[column]


def hll_aggs(spec):
    """[(aggregation index, column, log2m)] of the spec's HLL aggregations."""
    return [(a, c, Q.hll_log2m(f)) for a, (f, c) in enumerate(spec.aggregations) if Q.is_hll(f)]


def model(seg, spec, key_values=None, match=None):
    """{aggregation index: uint8 registers} of every HLL aggregation, or -- GROUP BY -- {raw group id: {aggregation index: registers}} over
    the groups that hold a matching doc.  match: the matching docs as bool[num_docs] where the oracle cannot evaluate the filter (a doc-set leaf)."""
    match = D.matching_docs(seg, spec) if match is None else np.asarray(match, dtype=bool)
    aggs = hll_aggs(spec)
    if not spec.group_by:
        return {a: registers(values_of(seg, c)[match], numpy_dtype_of(seg.columns[c]), log2m) for a, c, log2m in aggs}
    gid = D.group_ids_of(seg, spec, key_values)[match]
    order = np.argsort(gid, kind="stable")
    bounds = np.flatnonzero(np.diff(gid[order])) + 1
    matched = {c: values_of(seg, c)[match] for _, c, _ in aggs}
    out = {}
    for rows in np.split(order, bounds) if gid.shape[0] else []:
        out[int(gid[rows[0]])] = {a: registers(matched[c][rows], numpy_dtype_of(seg.columns[c]), log2m) for a, c, log2m in aggs}
    return out


def without_hll(spec):
    """The spec the oracle can run: every HLL turned into COUNT(*)."""
    aggs = [((Q.COUNT, -1) if Q.is_hll(f) else (f, c)) for f, c in spec.aggregations]
    return Q.QuerySpec(aggs, filter=spec.filter, group_by=spec.group_by, null_handling=spec.null_handling, num_groups_limit=spec.num_groups_limit,
                       stats_upper_bound_ok=spec.stats_upper_bound_ok)


def assert_registers_equal(got, seg, spec, want=None, key_values=None, where="", match=None):
    """The result's HLL fields against the model: the registers byte for byte, count = the non-zero registers, sum 0, min +inf, max -inf."""
    want = model(seg, spec, key_values, match) if want is None else want

    def one(v, regs, at):
        assert v.hll_registers is not None, "%s %s: no registers came back" % (where, at)
        got_regs = np.frombuffer(bytes(v.hll_registers), dtype=np.uint8)
        assert got_regs.shape == regs.shape, "%s %s: %d registers, model %d" % (where, at, got_regs.shape[0], regs.shape[0])
        bad = np.flatnonzero(got_regs != regs)
        assert bad.size == 0, "%s %s: %d registers differ, first %d: %d, model %d" % (where, at, bad.size, bad[0], got_regs[bad[0]], regs[bad[0]])
        assert v.count == int(np.count_nonzero(regs)) and v.sum == 0.0 and v.sum_i64 == 0 and not v.sum_exact and v.min == float("inf") and v.max == float("-inf"), (where, at, v)

    if not spec.group_by:
        for a, regs in want.items():
            one(got.aggregations[a], regs, "agg %d" % a)
        return
    assert sorted(got.groups) == sorted(want), "%s: groups differ (%d, model %d)" % (where, len(got.groups), len(want))
    for gid, sets in want.items():
        for a, regs in sets.items():
            one(got.groups[gid][a], regs, "group %d agg %d" % (gid, a))


def golden_spec(seg, filtered, grouped, filter_form="logical"):
    """One of testDistinctCountHLL's four queries on H.golden_segment() (or its raw-column variant: same column names)."""
    base = D.golden_spec(seg, filtered, grouped, filter_form)
    return Q.QuerySpec([(Q.hll(), c) for _, c in base.aggregations], filter=base.filter, group_by=base.group_by)


def golden_pair(sets):
    """(v1, v2) of a model / result row: the estimates of aggregations 0 and 1."""
    return cardinality(sets[0]), cardinality(sets[1])


# ---- synthetic segments of the edge tests ----
def typed_dict_column(S, name, dict_values, dict_ids):
    """A dictionary column over hand-made dictionary values of any numeric dtype, in the order given (the caller sorts them the way
    SegmentDictionaryCreator does -- Double.compare's order keeps -0.0 and 0.0 apart, which np.unique does not)."""
    from pinot_amd import _abi
    lib = S.load_host_library()
    dict_values = np.ascontiguousarray(dict_values)
    if dict_values.dtype == np.int32:
        return S.Column.from_dict_ids(name, dict_values, dict_ids)
    dict_ids = np.ascontiguousarray(dict_ids, dtype=np.int32)
    card, n = int(dict_values.shape[0]), int(dict_ids.shape[0])
    bits = int(lib.ph_num_bits_per_value(card - 1))
    fwd = np.zeros(int(lib.ph_fixedbit_size(n, bits)), dtype=np.uint8)
    if n:
        lib.ph_fixedbit_pack(S._i32p(dict_ids), n, bits, S._u8p(fwd), S.host_threads())
    dictionary = np.zeros(card * dict_values.dtype.itemsize, dtype=np.uint8)
    lib.ph_dict_write_fixed(dict_values.ctypes.data, card, dict_values.dtype.itemsize, S._u8p(dictionary))
    return S.Column(name, _abi.PG_FWD_FIXED_BIT_DICT, bits, card, fwd, dictionary, None, dict_values, stored_type=S.stored_type_of(dict_values.dtype))


def _sorted_like_java(values):
    """Distinct values by BIT PATTERN, ascending in Long.compare / Double.compare's order (-0.0 below 0.0, NaN last)."""
    values = np.ascontiguousarray(values)
    if values.dtype.kind != "f":
        return np.unique(values)
    as_int = values.view(np.int32 if values.dtype == np.float32 else np.int64)
    distinct = np.unique(as_int)
    # the order image of an IEEE value: flip the magnitude bits of negatives
    key = np.where(distinct < 0, distinct ^ np.iinfo(distinct.dtype).max, distinct)
    return distinct[np.argsort(key, kind="stable")].view(values.dtype)


EDGE_SIZES = [1, 33, 2047, 2049, 100003]
# column indexes of edge_segment
E_INT, E_LONG, E_FLOAT, E_DOUBLE, E_FILTER, E_K1, E_K2, E_ONE, E_SET = range(9)


def edge_segment(S, num_docs, raw, seed=11):
    """Four value columns of the four stored types -- raw, or dictionary-encoded -- with the values an HLL can get wrong: INT with negatives,
    LONG beyond 32 bits of both signs, FLOAT and DOUBLE with -0.0, 0.0 and NaNs of non-default payloads (a raw column holds two payloads, a
    sorted dictionary can hold one NaN); a filter column with an inverted index, two key columns, a column of one value, a column for IN lists."""
    rng = np.random.default_rng(seed + num_docs)
    n = num_docs
    pick = lambda pool: pool[rng.integers(0, len(pool), n)]
    ints = pick(np.concatenate([rng.integers(-2 ** 31, 2 ** 31, 3000), [-1, 0, 1, -2 ** 31, 2 ** 31 - 1]]).astype(np.int32))
    longs = pick(np.concatenate([rng.integers(-2 ** 62, 2 ** 62, 3000), [-1, 0, 2 ** 32, -2 ** 32 - 1, 2 ** 63 - 1, -2 ** 63]]).astype(np.int64))
    f_special = np.array([0x80000000, 0x00000000, 0x7FC00001, 0x7FC12345 if raw else 0x7FC00001, 0x7F800000, 0xFF800000], dtype=np.uint32).view(np.float32)
    d_special = np.array([0x8000000000000000, 0, 0x7FF8000000000001, 0x7FF80000DEADBEEF if raw else 0x7FF8000000000001, 0x7FF0000000000000], dtype=np.uint64).view(np.float64)
    floats = pick(np.concatenate([(rng.standard_normal(2000) * 1e3).astype(np.float32), f_special]))
    doubles = pick(np.concatenate([rng.standard_normal(2000) * 1e9, d_special]))
    if n >= 6:      # the special values are present whatever the draw
        floats[:6] = f_special
        doubles[:5] = d_special
    one = np.full(n, -77, dtype=np.int32)
    values = [ints, longs, floats, doubles]
    cols = []
    for name, v in zip("ilfd", values):
        if raw:
            cols.append(S.Column.raw_typed(name, v))
        else:
            dict_values = _sorted_like_java(v)
            bits_of = lambda a: a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
            order = np.argsort(bits_of(dict_values), kind="stable")
            ids = order[np.searchsorted(bits_of(dict_values)[order], bits_of(v))].astype(np.int32)
            cols.append(typed_dict_column(S, name, dict_values, ids))
    ids = lambda card: rng.integers(0, card, n).astype(np.int32)
    cols.append(S.Column.from_dict_ids("flt", np.arange(1000, dtype=np.int32), ids(1000), with_inverted=True))
    cols.append(S.Column.from_dict_ids("k1", np.arange(7, dtype=np.int32) * 3, ids(7)))
    cols.append(S.Column.from_dict_ids("k2", np.arange(5, dtype=np.int32) - 2, ids(5)))
    cols.append(S.Column.raw_typed("one", one) if raw else S.Column.from_dict_ids("one", np.array([-77], dtype=np.int32), np.zeros(n, dtype=np.int32)))
    cols.append(S.Column.from_dict_ids("s", np.arange(300, dtype=np.int32) * 11, ids(300)))
    seg = S.SegmentData("hll_edges_%d_%s" % (n, "raw" if raw else "dict"), n, cols)
    for c, v in zip((E_INT, E_LONG, E_FLOAT, E_DOUBLE, E_ONE), values + [one]):
        set_values(seg, c, v)
    return seg
