"""Shared builders and the exact model of the tests of PERCENTILE / DISTINCTCOUNT on raw (no-dictionary) columns (tests/test_raw_values_cpu.py,
tests/test_gpu_raw_values.py, tools/kernel_coverage.py, tools/bench_variants.py).

The model is not the oracle (which knows neither function): per aggregation -- and per raw group id -- it is
`np.unique(values[matching], return_counts=True)` in the ORDER IMAGE's order, with `matching` from `oracle.filter_bitmap`.  The order image
is the engine's sort key (pinot_amd/csrc/pg_order_image.h): INT / LONG  v ^ 2^63;  FLOAT (widened exactly) / DOUBLE  bits >= 0 ? bits | 2^63
: ~bits with every NaN the canonical one -- Double.compare's order.  What comes back is the value's BITS (pg_result_value_counts): the long
value of INT / LONG, the IEEE-754 bits of the double of FLOAT / DOUBLE.  Everything is compared exactly, pair for pair.
"""
import numpy as np

import distinct_cases as DC
from pinot_amd import query as Q

matching_docs = DC.matching_docs
group_ids_of = DC.group_ids_of
projected_columns = DC.projected_columns

SIGN = np.uint64(1 << 63)
CANONICAL_NAN = np.uint64(0x7FF8000000000000)
RAW_FUNCTIONS = (Q.PERCENTILE, Q.DISTINCTCOUNT)


def order_image(values):
    """uint64 order images of an int32 / int64 / float32 / float64 array."""
    values = np.asarray(values)
    if np.issubdtype(values.dtype, np.integer):
        return values.astype(np.int64).view(np.uint64) ^ SIGN
    with np.errstate(invalid="ignore"):                            # (a signalling NaN is quieted by the widening: it is canonicalised below anyway)
        bits = values.astype(np.float64).view(np.uint64).copy()   # (float32 -> float64 is exact)
    bits[(bits & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)] = CANONICAL_NAN
    negative = (bits >> np.uint64(63)) != 0
    return np.where(negative, ~bits, bits | SIGN)


def value_bits_of_image(images, floating):
    """int64 value bits behind order images: the way back (rank_image_value_bits)."""
    images = np.asarray(images, dtype=np.uint64)
    if not floating:
        return (images ^ SIGN).view(np.int64)
    positive = (images >> np.uint64(63)) != 0
    return np.where(positive, images & ~SIGN, ~images).view(np.int64)


def runs_of(values):
    """(ascending value bits int64, counts uint32) of an array of one stored type: the model of one list."""
    values = np.asarray(values)
    floating = np.issubdtype(values.dtype, np.floating)
    images, counts = np.unique(order_image(values), return_counts=True)
    return value_bits_of_image(images, floating), counts.astype(np.uint32)


def raw_aggregations(spec):
    return [(a, f, c) for a, (f, c) in enumerate(spec.aggregations) if f in RAW_FUNCTIONS]


def model(seg, spec, match=None, key_values=None):
    """{aggregation index: (value bits, counts)} of every PERCENTILE / DISTINCTCOUNT aggregation (seg.raw_values[column] holds the column's
    values), or -- GROUP BY -- {raw group id: {...}} over the groups that hold a matching doc.  match: the matching docs when the filter holds a
    leaf the oracle does not evaluate (a doc set), else oracle.filter_bitmap's."""
    match = matching_docs(seg, spec) if match is None else np.asarray(match, dtype=bool)
    aggs = raw_aggregations(spec)
    if not spec.group_by:
        return {a: runs_of(seg.raw_values[c][match]) for a, _, c in aggs}
    gid = group_ids_of(seg, spec, key_values)[match]
    order = np.argsort(gid, kind="stable")
    bounds = np.flatnonzero(np.diff(gid[order])) + 1
    matched = {c: seg.raw_values[c][match] for _, _, c in aggs}
    out = {}
    for rows in np.split(order, bounds) if gid.shape[0] else []:
        out[int(gid[rows[0]])] = {a: runs_of(matched[c][rows]) for a, _, c in aggs}
    return out


def without_raw_functions(spec):
    """The spec the oracle can run: every PERCENTILE / DISTINCTCOUNT turned into COUNT(*)."""
    aggs = [((Q.COUNT, -1) if f in RAW_FUNCTIONS else (f, c)) for f, c in spec.aggregations]
    return Q.QuerySpec(aggs, filter=spec.filter, group_by=spec.group_by, null_handling=spec.null_handling, num_groups_limit=spec.num_groups_limit,
                       stats_upper_bound_ok=spec.stats_upper_bound_ok)


def assert_lists_equal(got, spec, want, where=""):
    """The result's PERCENTILE / DISTINCTCOUNT fields against the model: the runs pair for pair; count = the list's length (PERCENTILE) or the
    number of runs (DISTINCTCOUNT), sum 0, min +inf, max -inf; no dictionary form beside them."""
    functions = {a: f for a, f, _ in raw_aggregations(spec)}

    def one(v, pairs, a, at):
        assert v.value_counts is not None, "%s %s: no value list came back" % (where, at)
        assert v.dict_ids is None and v.dict_id_counts is None
        bits, counts = v.value_counts
        assert bits.dtype == np.int64 and counts.dtype == np.uint32
        assert np.array_equal(bits, pairs[0]), "%s %s: values differ (%d runs, model %d)" % (where, at, len(bits), len(pairs[0]))
        assert np.array_equal(counts, pairs[1]), "%s %s: counts differ" % (where, at)
        want_count = int(pairs[1].astype(np.int64).sum()) if functions[a] == Q.PERCENTILE else len(pairs[0])
        assert v.count == want_count, (where, at, v.count, want_count)
        assert v.sum == 0.0 and v.sum_i64 == 0 and not v.sum_exact and v.min == float("inf") and v.max == float("-inf"), (where, at, v)

    if not spec.group_by:
        for a, pairs in want.items():
            one(got.aggregations[a], pairs, a, "agg %d" % a)
        return
    assert sorted(got.groups) == sorted(want), "%s: groups differ (%d, model %d)" % (where, len(got.groups), len(want))
    for gid, lists in want.items():
        for a, pairs in lists.items():
            one(got.groups[gid][a], pairs, a, "group %d agg %d" % (gid, a))


def assert_other_functions_equal(got, seg, spec):
    """Every function of the query that is neither, and the statistics, against the unchanged oracle."""
    import helpers as H
    from oracle import oracle
    want = oracle.execute(seg, without_raw_functions(spec))
    for a, (f, _) in enumerate(spec.aggregations):
        if f in RAW_FUNCTIONS:
            continue
        if spec.group_by:
            for gid in want.groups:
                H.assert_agg_equal(got.groups[gid][a], want.groups[gid][a], f, "group %r agg %d" % (gid, a))
                assert got.groups[gid][a].value_counts is None
        else:
            H.assert_agg_equal(got.aggregations[a], want.aggregations[a], f, "agg %d" % a)
            assert got.aggregations[a].value_counts is None
    if spec.group_by:
        assert sorted(got.groups) == sorted(want.groups), "group ids differ"
    assert got.stats[0] == want.stats[0] and got.stats[3] == want.stats[3], (got.stats, want.stats)
    assert got.stats[2] == got.stats[0] * projected_columns(spec), (got.stats, projected_columns(spec))
    if got.filter_entries_exact and want.filter_entries_exact:
        assert got.stats[1] == want.stats[1], (got.stats, want.stats)


def same_lists(one, other, spec):
    """Two results of the same query hold identical lists (slot order on the device differs from run to run; the sort removes it)."""
    rows = lambda r: [r.aggregations] if not spec.group_by else [r.groups[g] for g in sorted(r.groups)]
    assert sorted(one.groups) == sorted(other.groups) and one.stats == other.stats
    for ra, rb in zip(rows(one), rows(other)):
        for a, _, _ in raw_aggregations(spec):
            assert ra[a].count == rb[a].count
            assert np.array_equal(ra[a].value_counts[0], rb[a].value_counts[0]) and np.array_equal(ra[a].value_counts[1], rb[a].value_counts[1])


# ---- the values a merge sees (pinot_host.h: ValueCounts / ValueSet) ----
def double_of_bits(bits, stored_type_floating):
    """getDoubleValuesSV over value bits: (double) of the long for INT / LONG, the double itself for FLOAT / DOUBLE."""
    bits = np.asarray(bits, dtype=np.int64)
    return bits.view(np.float64) if stored_type_floating else bits.astype(np.float64)


# ---- segments ----
TILE = 2048
EDGE_SIZES = (1, 31, 32, 33, 2047, 2048, 2049, 3 * 2048 + 37)
PATTERNS = ("none", "all", "lane0", "lane63-last", "one-per-tile", "alternating", "one-tile", "tile-list", "doc-set", "in-list")


def pattern_mask(pattern, n):
    """bool[n]: the docs a match pattern names, on the kernel's geometry (a wave per 2048-doc tile, lane l its docs 32 l .. 32 l + 31)."""
    d = np.arange(n)
    in_tile = d % TILE
    if pattern == "none":
        return np.zeros(n, dtype=bool)
    if pattern == "all":
        return np.ones(n, dtype=bool)
    if pattern == "lane0":
        return in_tile < 32
    if pattern == "lane63-last":
        return in_tile == TILE - 1
    if pattern == "one-per-tile":
        return in_tile == (37 * (d // TILE) + 5) % TILE
    if pattern == "alternating":
        return d % 2 == 1
    if pattern == "one-tile":
        return d // TILE == (1 if n > TILE else 0)
    # the three leaf kinds: a pseudo-random third of the docs, the same for each
    return (np.random.default_rng(n).random(n) < 0.33)


def edge_segment(S, n, pattern, seed=3):
    """`n` docs, four raw columns of the four stored types (columns 0-3: INT, LONG, FLOAT, DOUBLE), and the filter columns that express
    `pattern`: 4 `m` (dictId 1 where the doc matches, inverted index beside it), 5 `s` (cardinality 40: the IN list takes the dictIds of the
    matching docs, which no other doc carries).  seg.mask: the pattern; seg.raw_values: the columns' values."""
    rng = np.random.default_rng(seed * 100003 + n)
    mask = pattern_mask(pattern, n)
    vi = rng.integers(-50, 50, n).astype(np.int32)
    vl = (rng.integers(-2000, 2000, n).astype(np.int64)) * ((1 << 33) + 7)
    vf = (rng.integers(-40, 40, n).astype(np.float32)) * np.float32(0.25)
    vd = rng.integers(-3000, 3000, n).astype(np.float64) * 0.37
    s_ids = np.where(mask, rng.integers(0, 17, n), rng.integers(17, 40, n)).astype(np.int32)
    cols = [S.Column.raw("ri", vi), S.Column.raw_typed("rl", vl), S.Column.raw_typed("rf", vf), S.Column.raw_typed("rd", vd),
            S.Column.from_dict_ids("m", np.arange(2, dtype=np.int32), mask.astype(np.int32), with_inverted=True),
            S.Column.from_dict_ids("s", np.arange(40, dtype=np.int32), s_ids)]
    seg = S.SegmentData("raw_edge_%d_%s" % (n, pattern), n, cols)
    seg.mask = mask
    seg.raw_values = {0: vi, 1: vl, 2: vf, 3: vd}
    return seg


def edge_filter(pattern, doc_set_id=None):
    """The filter that matches seg.mask: a dictionary range leaf, or the leaf kind the pattern is named after."""
    if pattern == "tile-list":
        return Q.leaf(Q.Pred.dict_range(4, 1, 2, inverted=True))
    if pattern == "doc-set":
        return Q.leaf(Q.Pred.doc_set(doc_set_id))
    if pattern == "in-list":
        return Q.leaf(Q.Pred.dict_set(5, list(range(17)), 40))
    return Q.leaf(Q.Pred.dict_range(4, 1, 2))
