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


def assert_one_register_set(v, regs, where=""):
    """One AggValue of an HLL aggregation: the registers byte for byte, count = the non-zero registers, sum 0, min +inf, max -inf."""
    assert v.hll_registers is not None, "%s: no registers came back" % where
    got_regs = np.frombuffer(bytes(v.hll_registers), dtype=np.uint8)
    assert got_regs.shape == regs.shape, "%s: %d registers, model %d" % (where, got_regs.shape[0], regs.shape[0])
    bad = np.flatnonzero(got_regs != regs)
    assert bad.size == 0, "%s: %d registers differ, first %d: %d, model %d" % (where, bad.size, bad[0], got_regs[bad[0]], regs[bad[0]])
    assert v.count == int(np.count_nonzero(regs)) and v.sum == 0.0 and v.sum_i64 == 0 and not v.sum_exact and v.min == float("inf") and v.max == float("-inf"), (where, v)


def assert_registers_equal(got, seg, spec, want=None, key_values=None, where="", match=None):
    """The result's HLL fields against the model: the registers byte for byte, count = the non-zero registers, sum 0, min +inf, max -inf."""
    want = model(seg, spec, key_values, match) if want is None else want
    one = lambda v, regs, at: assert_one_register_set(v, regs, "%s %s" % (where, at))

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


# ---- constructed register corpus: values whose hash is chosen ----
M_INVERSE = np.uint32(pow(0x5BD1E995, -1, 1 << 32))                     # the constant is odd: multiplication by it is a bijection mod 2^32
CORPUS_LOG2M = (4, 8, 14)
CORPUS_SIZES = (2049, 6145)
C_INT, C_LONG, C_FLOAT, C_DOUBLE, C_FILTER, C_KEY = range(6)
CORPUS_RUN = 64                                                         # consecutive docs of one value: a whole wavefront offers one register at once


def _undo_xor_shift(y, s):
    """x of y = x ^ (x >> s), 32 bits: the top s bits of x are y's, every pass restores s more."""
    x = int(y)
    for _ in range(32 // s + 1):
        x = int(y) ^ (x >> s)
    return x & 0xFFFFFFFF


def long_with_hash(x, hi):
    """The long with high word `hi` whose hash_long is x: every Murmur2 step undone, last to first."""
    m, inv, mask = int(M), int(M_INVERSE), 0xFFFFFFFF
    h = _undo_xor_shift(int(x) & mask, 15)
    h = (h * inv) & mask
    h = _undo_xor_shift(h, 13)
    k = ((int(hi) & mask) * m) & mask
    k ^= k >> 24
    h ^= (k * m) & mask
    h = (h * inv) & mask                                                # = (k_low * M): the first word's contribution
    k = (h * inv) & mask
    k = _undo_xor_shift(k, 24)
    lo = (k * inv) & mask
    v = ((int(hi) & mask) << 32) | lo
    return v - (1 << 64) if v >= 1 << 63 else v


def int_with_hash(x):
    """The int (as a Python integer) whose sign-extended long hashes to x, or None: the high word of a sign-extended int is 0 or -1, and the
    low word that solves the hash for it must carry the same sign."""
    for hi in (0, -1):
        v = long_with_hash(x, hi)
        if -2 ** 31 <= v < 2 ** 31:
            return v
    return None


def hash_of_target(log2m, index, rank):
    """The hash that lands in register `index` with rank `rank`, its remainder all zero below the leading one (rank max: all zero, so that
    only the sentinel bit ends the count)."""
    rest = 32 - log2m
    assert 0 <= index < 1 << log2m and 1 <= rank <= rest + 1
    return (index << rest) | (0 if rank == rest + 1 else 1 << (rest - rank))


def corpus_targets(log2m):
    """[(index, rank)]: the first, one middle and the last register, each with rank 1, 2, max - 1 and max = 32 - log2m + 1."""
    m, top = 1 << log2m, 32 - log2m + 1
    return [(j, r) for j in (0, (m // 2) | 5 if m > 16 else 5, m - 1) for r in (1, 2, top - 1, top)]


def corpus_values(width):
    """{(log2m, index, rank): value} -- 64-bit longs (width 64: the index is always reached) or ints (width 32: where an index has no 32-bit
    solution, the nearest index that has one).  `index` is the one reached."""
    out = {}
    for log2m in CORPUS_LOG2M:
        m = 1 << log2m
        for j, r in corpus_targets(log2m):
            if width == 64:
                # a high word of every shape, fixed per target
                out[(log2m, j, r)] = long_with_hash(hash_of_target(log2m, j, r), (0x9E3779B9 * (j + 3 * r + log2m)) & 0xFFFFFFFF)
                continue
            for d in sorted(range(m), key=lambda d: (abs(d - j), d)):
                v = int_with_hash(hash_of_target(log2m, d, r))
                if v is not None:
                    out[(log2m, d, r)] = v
                    break
    return out


def corpus_order(n, targets):
    """Doc -> position in `targets`.  Per register the entries go [largest rank, smaller ranks ..., largest rank], so the largest rank is
    offered both before and after the smaller ones (the plain read before the atomic max must survive both orders); the registers' entries
    are cycled in short runs over the docs.  Three runs of CORPUS_RUN consecutive docs carry a largest-rank value: at doc 0, across the
    middle of tile 1, and ending in the last doc.  A lane holds 32 consecutive docs, so in the third tile (when there is a whole one) the
    cycle has a period of 32 docs instead: all 64 lanes of the wavefront then offer the same register in the same step."""
    per_register = {}
    for i, (log2m, j, r) in enumerate(targets):
        per_register.setdefault((log2m, j), []).append((r, i))
    groups, largest = [], []
    for entries in per_register.values():
        entries = sorted(entries, reverse=True)
        groups.append([entries[0][1]] + [i for _, i in entries[1:]] + [entries[0][1]])
        largest.append(entries[0][1])

    def whole_groups(room, repeat):
        """Whole groups (never one cut short) in cycle, every entry `repeat` docs long, padded to `room` docs with the last group's largest rank."""
        out, k = [], 0
        while len(out) + len(groups[k % len(groups)]) * repeat <= room:
            out += [i for i in groups[k % len(groups)] for _ in range(repeat)]
            k += 1
        return np.array(out + [out[-1]] * (room - len(out)), dtype=np.int64)

    docs = np.empty(n, dtype=np.int64)
    docs[:CORPUS_RUN] = largest[0]
    body_end = 2 * 2048 if n >= 3 * 2048 else n - CORPUS_RUN
    docs[CORPUS_RUN: body_end] = whole_groups(body_end - CORPUS_RUN, 5)
    if n >= 3 * 2048:
        docs[2 * 2048: n] = np.tile(whole_groups(32, 1), -(-(n - 2 * 2048) // 32))[: n - 2 * 2048]
    mid = 2048 + 1024 if n > 2048 + 1024 + CORPUS_RUN else n // 2
    docs[mid - CORPUS_RUN // 2: mid + CORPUS_RUN // 2] = largest[len(largest) // 2]
    docs[n - CORPUS_RUN:] = largest[-1]
    return docs


def corpus_segment(S, num_docs, raw):
    """INT / LONG / FLOAT (the constructed 32 bits as float bits) / DOUBLE (the constructed 64 bits) columns over the constructed values, a
    filter column and a 5-value key.  NaN bit patterns stay in raw columns only (a widened FLOAT dictionary quiets a signalling NaN and a
    sorted dictionary holds one NaN): the dictionary form replaces them by the column's first non-NaN value."""
    n = num_docs
    rng = np.random.default_rng(41 + n)
    wide, narrow = corpus_values(64), corpus_values(32)
    columns, stored = [], []
    for name, width, dtype in (("i", 32, np.int32), ("l", 64, np.int64), ("f", 32, np.float32), ("d", 64, np.float64)):
        table = narrow if width == 32 else wide
        targets = list(table)
        ints = np.array([table[t] for t in targets], dtype=np.int32 if width == 32 else np.int64)
        values = ints[corpus_order(n, targets)].view(dtype)
        if dtype in (np.float32, np.float64) and not raw:
            nan = np.isnan(values)
            values = np.where(nan, values[~nan][0], values).astype(dtype)
        stored.append(np.ascontiguousarray(values))
    for name, v in zip("ilfd", stored):
        if raw:
            columns.append(S.Column.raw_typed(name, v))
        else:
            dict_values = _sorted_like_java(v)
            bits_of = lambda a: a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
            order = np.argsort(bits_of(dict_values), kind="stable")
            ids = order[np.searchsorted(bits_of(dict_values)[order], bits_of(v))].astype(np.int32)
            columns.append(typed_dict_column(S, name, dict_values, ids))
    columns.append(S.Column.from_dict_ids("flt", np.arange(1000, dtype=np.int32), rng.integers(0, 1000, n).astype(np.int32)))
    columns.append(S.Column.from_dict_ids("k", np.arange(5, dtype=np.int32) * 2 - 3, rng.integers(0, 5, n).astype(np.int32)))
    seg = S.SegmentData("hll_corpus_%d_%s" % (n, "raw" if raw else "dict"), n, columns)
    for c, v in zip((C_INT, C_LONG, C_FLOAT, C_DOUBLE), stored):
        set_values(seg, c, v)
    return seg


# ---- fold edges: chosen dictIds around hll_fold_kernel's chunks ----
FOLD_CARDINALITIES = (8191, 8192, 8193, 8225, 16385, 524288, 524289)
FOLD_DOCS = 4097
F_INT, F_LONG, F_FILTER, F_KEY = range(4)


def fold_chunks(cardinality):
    """[(first word, end word)] of the chunks launch_hll_fold forms (restated, not called): one workgroup per 256 words of a bitset row, at
    most 64, then the words per chunk by ceiling division."""
    words = (cardinality + 31) // 32
    chunks = max(1, min(64, (words + 255) // 256))
    per = (words + chunks - 1) // chunks
    return [(c * per, min(words, (c + 1) * per)) for c in range(chunks) if c * per < words]


def fold_dict_ids(cardinality):
    """(dictIds, chunk of each): the first and last dictId of EVERY chunk, two interior ones per chunk, and cardinality - 1 (the last
    chunk's last: a cardinality that is no multiple of 32 has it in a partial word)."""
    ids = {}
    for c, (first, end) in enumerate(fold_chunks(cardinality)):
        lo, hi = first * 32, min(cardinality, end * 32) - 1
        for d in (lo, hi, lo + (hi - lo) // 2, min(hi, lo + 33)):
            ids[d] = c
    assert cardinality - 1 in ids
    order = sorted(ids)
    return np.array(order, dtype=np.int32), np.array([ids[d] for d in order], dtype=np.int32)


FOLD_ALL, FOLD_ODD, FOLD_EVEN = (1, 3), (2, 3), (1, 2)                  # dictId ranges [lo, hi) of the filter column, below


def fold_segment(S, cardinality):
    """Dictionary INT and LONG columns of the given cardinality whose docs carry exactly fold_dict_ids (in a fixed shuffled order); a filter
    column whose dictId is 1 for a doc of an even chunk, 2 for a doc of an odd chunk and 9 for the last doc -- so a range leaf can keep every
    chunk (FOLD_ALL), or leave the even / the odd chunks wholly without a bit (FOLD_ODD / FOLD_EVEN); a 5-value key."""
    n = FOLD_DOCS
    rng = np.random.default_rng(cardinality)
    chosen, chunk_of = fold_dict_ids(cardinality)
    pick = rng.permutation(n) % len(chosen)
    ids = chosen[pick].astype(np.int32)
    flt = (1 + chunk_of[pick] % 2).astype(np.int32)
    flt[-1] = 9
    ints = (np.arange(cardinality, dtype=np.int64) * 3 - 700000).astype(np.int32)
    longs = np.arange(cardinality, dtype=np.int64) * 0x100000003 - 2 ** 50
    cols = [S.Column.from_dict_ids("i", ints, ids), typed_dict_column(S, "l", longs, ids),
            S.Column.from_dict_ids("flt", np.arange(10, dtype=np.int32), flt),
            S.Column.from_dict_ids("k", np.arange(5, dtype=np.int32), rng.integers(0, 5, n).astype(np.int32))]
    return S.SegmentData("hll_fold_%d" % cardinality, n, cols)
