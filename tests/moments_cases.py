"""VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP: what the tests of PG_AGG_VARIANCE share.

An exact model (integer arithmetic over the doubles the values convert to), a restatement of the reference's own arithmetic
(VarianceTuple.apply per doc inside 10 000-doc blocks, block tuples merged in order), the value families, the derived tolerance and the segment
builders.  Nothing here runs on a device."""
import math
from fractions import Fraction

import numpy as np

import distinct_cases as D
import hll_cases as HL
from pinot_amd import query as Q

U = Fraction(1, 2 ** 53)
BLOCK_DOCS = 10000      # DocIdSetPlanNode.MAX_DOC_PER_CALL: the docs one aggregate() call sees
SIZES = [1, 2, 33, 2047, 2049, 100003]
BIG = 100003


# ---- the value families: name -> (numpy dtype, values(rng, n)) ----
def _const(value, dtype):
    return lambda rng, n: np.full(n, value, dtype=dtype)


FAMILIES = {
    "int_uniform": (np.int32, lambda rng, n: rng.integers(0, 500, n).astype(np.int32)),
    "double_pm1e6": (np.float64, lambda rng, n: rng.uniform(-1e6, 1e6, n)),
    "long_1p7e12": (np.int64, lambda rng, n: (1700000000000 + rng.integers(0, 3600000, n)).astype(np.int64)),
    "float_normal": (np.float32, lambda rng, n: rng.standard_normal(n).astype(np.float32)),
    "int_const7": (np.int32, _const(7, np.int32)),
    "int_full": (np.int32, lambda rng, n: rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)),
    "double_unit": (np.float64, lambda rng, n: rng.uniform(0.0, 1.0, n)),
    "long_2p62": (np.int64, lambda rng, n: (2 ** 62 + rng.integers(0, 2 ** 20, n)).astype(np.int64)),
    "double_const01": (np.float64, _const(0.1, np.float64)),
    # (not one of the reference's parity or beyond families: a LONG dictionary too wide for 32-bit offsets, so that every value source is read)
    "long_wide": (np.int64, lambda rng, n: rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64)),
}
# the restated reference stays inside tol(...) of exact on these at 100 003 docs ...
PARITY = ["int_uniform", "double_pm1e6", "long_1p7e12", "float_normal", "int_const7"]
# ... and on these at the sizes named
PARITY_SMALL = [("int_full", 1), ("int_full", 2), ("int_full", 33), ("double_unit", 2049)]
# ... and leaves it on these: they are held against the exact model only
BEYOND = ["long_2p62", "double_const01"]
VALUE_COLUMNS = list(FAMILIES)
C_FILTER, C_K1, C_K2, C_SET = (len(VALUE_COLUMNS) + i for i in range(4))


def family_values(name, n, seed=0):
    dtype, make = FAMILIES[name]
    # (a seed per family and size, independent of Python's string hashing)
    return np.ascontiguousarray(make(np.random.default_rng([seed, VALUE_COLUMNS.index(name), n]), n), dtype=dtype)


def as_doubles(values):
    """StatisticalAggregationFunctionUtils.getValSet: (double) of the int / long / float."""
    return np.asarray(values).astype(np.float64)


# ---- the exact model ----
LIMB_BITS = 24
LIMB_MASK = (1 << LIMB_BITS) - 1
CHUNK = 4096      # products of two limbs are below 2^48: a chunk's sum stays below 2^60


class Exact:
    """The doubles of one column as integers V_i x 2^e over one exponent, V_i cut into signed 24-bit limbs held in int64 arrays: sums of the V_i
    and of their squares are exact (numpy adds limbs and limb products chunk by chunk, Python integers join the chunks)."""

    def __init__(self, doubles):
        doubles = np.ascontiguousarray(doubles, dtype=np.float64)
        assert np.all(np.isfinite(doubles))
        mant, exp = np.frexp(doubles)
        mant = (mant * 2.0 ** 53).astype(np.int64)      # exact: a double's mantissa has 53 bits
        exp = exp.astype(np.int64) - 53
        nonzero = mant != 0
        self.e = int(exp[nonzero].min()) if np.any(nonzero) else 0
        shift = np.where(nonzero, exp - self.e, 0)
        bits = 53 + (int(shift.max()) if shift.shape[0] else 0)
        assert bits <= 53 + 2100
        sign, mag = np.sign(mant), np.abs(mant)
        self.limbs = []
        for j in range((bits + LIMB_BITS - 1) // LIMB_BITS):
            t = LIMB_BITS * j - shift                     # limb j of mag << shift: bits [24 j, 24 j + 24) of it
            right = (mag >> np.clip(t, 0, 63)) & LIMB_MASK
            s = np.clip(-t, 0, LIMB_BITS)
            left = ((mag & (LIMB_MASK >> s)) << s) & LIMB_MASK
            self.limbs.append(sign * np.where(t >= 0, right, left))
        self.abs = np.abs(doubles)

    @staticmethod
    def _sum(a):
        """The exact sum of an int64 array whose elements are below 2^48 in magnitude."""
        head = (a.shape[0] // CHUNK) * CHUNK
        return sum(a[:head].reshape(-1, CHUNK).sum(axis=1).tolist()) + int(a[head:].sum())

    def moments(self, rows=None):
        """(n, sum x, E = sum x^2 - (sum x)^2 / n, max |x|) over the docs `rows` (a bool mask or an index array; None: all), as Fractions."""
        limbs = self.limbs if rows is None else [l[rows] for l in self.limbs]
        n = int(limbs[0].shape[0]) if limbs else 0
        if n == 0:
            return 0, Fraction(0), Fraction(0), Fraction(0)
        s = sum(self._sum(l) << (LIMB_BITS * j) for j, l in enumerate(limbs))
        q = 0
        for j, a in enumerate(limbs):
            for k in range(j, len(limbs)):
                q += (self._sum(a * limbs[k]) * (1 if j == k else 2)) << (LIMB_BITS * (j + k))
        scale = Fraction(2) ** self.e
        x_max = Fraction(float((self.abs if rows is None else self.abs[rows]).max()))
        return n, s * scale, (Fraction(q) - Fraction(s * s, n)) * scale * scale, x_max


def tol(n, e, x_max):
    """|m2 - E| the two-run scheme may leave, u = 2^-53: 4 n u E bounds the error of S2 (n non-negative terms in any order, each with the
    roundings of x - c and its square), 4 n^2 u (n u X)^2 the error of the S1^2 / n correction when the pivot carries SUM's rounding (|c - mean|
    <= n u X, so |S1| <= n (n u X))."""
    return 4 * n * U * e + 4 * n * n * U * (n * U * x_max) ** 2


# ---- the reference's arithmetic, restated ----
def apply_value(t, value):
    """VarianceTuple.apply(double) :35-42."""
    count, total, m2 = t
    count += 1
    total += value
    if count > 1:
        d = count * value - total
        m2 += (d * d) / (count * (count - 1))
    return count, total, m2


def apply_tuple(t, other):
    """VarianceTuple.apply(VarianceTuple) :55-64 (and apply(long, double, double) :44-53, the same arithmetic)."""
    count, total, m2 = t
    o_count, o_total, o_m2 = other
    if o_count == 0:
        return t
    avg = 0.0 if count == 0 else total / count
    delta = (o_total / o_count) - avg
    m2 += o_m2 + delta * delta * o_count * count / (o_count + count)
    return count + o_count, total + o_total, m2


def reference_tuple(doubles, block_docs=BLOCK_DOCS):
    """VarianceAggregationFunction.aggregate :77-94 over the docs in order: a fresh tuple per block of block_docs, merged into the holder's."""
    doubles = [float(x) for x in np.asarray(doubles, dtype=np.float64)]
    holder = None
    for first in range(0, len(doubles), block_docs):
        t = (0, 0.0, 0.0)
        for x in doubles[first:first + block_docs]:
            t = apply_value(t, x)
        holder = t if holder is None else apply_tuple(holder, t)
    return holder if holder is not None else (0, 0.0, 0.0)


def merge_tuples(tuples):
    """The combine: the first block's tuple, every later one applied to it in order."""
    out = None
    for t in tuples:
        out = tuple(t) if out is None else apply_tuple(out, t)
    return out


def final(kind, t):
    """extractFinalResult :181-201; kind: varpop | varsamp | stddevpop | stddevsamp."""
    count, _, m2 = t
    sample = kind.endswith("samp")
    if count == 0 or (sample and count == 1):
        return float("-inf")
    v = m2 / (count - 1 if sample else count)
    return math.sqrt(v) if kind.startswith("stddev") else v


# ---- segments ----
def build_segment(S, num_docs, raw, seed=0):
    """Every family as a value column -- raw, or dictionary-encoded -- then a filter column with an inverted index, two key columns and a column
    for IN lists.  The model's copy of the values travels with the segment (values_of)."""
    n = num_docs
    rng = np.random.default_rng([seed, 99, n])
    cols, values = [], {}
    for c, name in enumerate(VALUE_COLUMNS):
        v = family_values(name, n, seed)
        values[c] = v
        if raw:
            cols.append(S.Column.raw_typed(name, v))
        else:
            dict_values = HL._sorted_like_java(v)
            cols.append(HL.typed_dict_column(S, name, dict_values, np.searchsorted(dict_values, v).astype(np.int32)))
    ids = lambda card: rng.integers(0, card, n).astype(np.int32)
    cols.append(S.Column.from_dict_ids("flt", np.arange(1000, dtype=np.int32), ids(1000), with_inverted=True))
    cols.append(S.Column.from_dict_ids("k1", np.arange(7, dtype=np.int32) * 3, ids(7)))
    cols.append(S.Column.from_dict_ids("k2", np.arange(5, dtype=np.int32) - 2, ids(5)))
    cols.append(S.Column.from_dict_ids("s", np.arange(300, dtype=np.int32) * 11, ids(300)))
    seg = S.SegmentData("moments_%d_%s" % (n, "raw" if raw else "dict"), n, cols)
    seg.__dict__["_moments_values"] = values
    seg.__dict__["_moments_exact"] = {}
    return seg


def values_of(seg, column):
    return seg.__dict__["_moments_values"][column]


def set_values(seg, column, values):
    seg.__dict__.setdefault("_moments_values", {})[column] = np.asarray(values)
    seg.__dict__.setdefault("_moments_exact", {}).pop(column, None)


def exact_of(seg, column):
    cache = seg.__dict__.setdefault("_moments_exact", {})
    if column not in cache:
        cache[column] = Exact(as_doubles(values_of(seg, column)))
    return cache[column]


def variance_aggs(spec):
    return [(a, c) for a, (f, c) in enumerate(spec.aggregations) if f == Q.VARIANCE]


def model(seg, spec, match=None):
    """{aggregation: (n, sum, E, X)} of every VARIANCE aggregation, or -- GROUP BY -- {raw group id: {aggregation: ...}} over the groups that hold a
    matching doc; over the docs oracle.filter_bitmap matches."""
    match = D.matching_docs(seg, spec) if match is None else np.asarray(match, dtype=bool)
    aggs = variance_aggs(spec)
    if not spec.group_by:
        return {a: exact_of(seg, c).moments(match) for a, c in aggs}
    docs = np.flatnonzero(match)
    gid = D.group_ids_of(seg, spec)[docs]
    order = np.argsort(gid, kind="stable")
    bounds = np.flatnonzero(np.diff(gid[order])) + 1
    out = {}
    for rows in np.split(order, bounds) if docs.shape[0] else []:
        out[int(gid[rows[0]])] = {a: exact_of(seg, c).moments(docs[rows]) for a, c in aggs}
    return out


def without_variance(spec):
    """The spec the oracle can run: every VARIANCE turned into COUNT(*)."""
    aggs = [((Q.COUNT, -1) if f == Q.VARIANCE else (f, c)) for f, c in spec.aggregations]
    return Q.QuerySpec(aggs, filter=spec.filter, group_by=spec.group_by, null_handling=spec.null_handling, num_groups_limit=spec.num_groups_limit,
                       stats_upper_bound_ok=spec.stats_upper_bound_ok)


def assert_one_tuple(v, want, sum_value=None, where="", quiet=False):
    """One AggValue of a VARIANCE aggregation against the exact model: count, |m2 - E| <= tol, m2 >= 0, min +inf, max -inf, and -- sum_value: the
    AggValue of a PG_AGG_SUM on the same column in the same query -- the sum fields bit for bit."""
    n, _, e, x_max = want
    assert v.moments is not None, "%s: no tuple came back" % where
    count, total, m2 = v.moments
    assert count == n == v.count, (where, count, n, v.count)
    assert total == v.sum or (total != total and v.sum != v.sum), (where, total, v.sum)
    assert v.min == float("inf") and v.max == float("-inf"), (where, v)
    bound = tol(n, e, x_max)
    if not quiet:
        print("%s: n=%d m2=%r E=%r |m2-E|=%.3e tol=%.3e" % (where, n, m2, float(e), float(abs(Fraction(m2) - e)), float(bound)))
    assert m2 >= 0.0, (where, m2)
    assert abs(Fraction(m2) - e) <= bound, "%s: m2 %r, exact %r: off by %.3e, tol %.3e" % (where, m2, float(e), float(abs(Fraction(m2) - e)), float(bound))
    if n == 0:
        assert m2 == 0.0, (where, m2)
    if sum_value is not None:
        assert (np.float64(v.sum).tobytes(), v.sum_i64, v.sum_exact) == (np.float64(sum_value.sum).tobytes(), sum_value.sum_i64, sum_value.sum_exact), (where, v, sum_value)


def assert_moments(got, seg, spec, where="", match=None, quiet=False):
    """Every VARIANCE aggregation of the result against the model; a (SUM, same column) aggregation of the spec is held bit-equal."""
    want = model(seg, spec, match)
    sum_at = {c: a for a, (f, c) in enumerate(spec.aggregations) if f == Q.SUM}

    def row(values, tuples, at):
        for a, c in variance_aggs(spec):
            assert_one_tuple(values[a], tuples[a], values[sum_at[c]] if c in sum_at else None, "%s %s agg %d (%s)" % (where, at, a, seg.columns[c].name), quiet)

    if not spec.group_by:
        row(got.aggregations, want, "")
        return want
    assert sorted(got.groups) == sorted(want), "%s: groups differ (%d, model %d)" % (where, len(got.groups), len(want))
    for gid, tuples in want.items():
        row(got.groups[gid], tuples, "group %d" % gid)
    return want
