"""Pinned edges of the partitioned group-by (pg_group_partition.h, run_partitioned_group_by): constructed segments of at most 140 000 docs
under PINOT_GPU_GROUP_PARTITION=force, on the whole device and on one CU, each query against the oracle AND a direct numpy group-by.
Every input is an integer (the one DOUBLE column holds multiples of 0.5), so every comparison is exact.

CASES names what each segment pins: key spaces on the partition boundaries and on the one-level / two-level switch at either shift;
doc counts around the 2048-doc tile, the 8192-doc scatter round and the 65 536-record chunk with one key per doc and with one key for all;
partitions and coarse partitions of more than one chunk, and chunks the filter leaves empty; the packed-record width boundary
(field + scatter shift = 32 / 33) at one and two levels, each once more with PINOT_GPU_PARTITION_PACKED=0; sign extension and the MIN / MAX
identities over -2^31 .. 2^31-1; three against four accumulators; the per-segment histogram cache across filters and shifts, once more
with PINOT_GPU_PARTITION_STATS_CACHE=0; one context through two-level, one-level and direct-table queries; numGroupsLimit below, at and
above the number of groups; one key space above 2^24.

Every query states the plan it is named for -- shift, log2 of the fine partitions per coarse one, whether it is partitioned, the packed
field width -- and test_every_case_took_the_plan_it_is_named_for reads the engine's own "group-by plan:" lines (PINOT_GPU_PARTITION_TRACE=1,
read once per process: hence a fresh child, which runs this file as a script) to confirm them."""
import collections
import os
import re
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fuzz_group_cases as G
import group_map_cases as GM
import helpers as H
from device_results import same_results
from oracle import oracle
from pinot_amd import query as Q
from pinot_amd import segment as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ["PINOT_GPU_GROUP_PARTITION", "PINOT_GPU_PARTITION_PACKED", "PINOT_GPU_PARTITION_STATS_CACHE", "PINOT_GPU_TEST_CUS"]

# One query of a case: aggregations as (function, column name or None), the case's filter by name, numGroupsLimit, and the plan it is
# named for: shift, log2_fine_per_coarse, partitioned or not, packed field width (0: separate key / value columns).
Query = collections.namedtuple("Query", "label aggs filter limit keys shift k partition packed")


def query(label, aggs, shift, k, packed, filter=None, limit=0, partition=True, keys=None):
    """keys: how many of the segment's key columns the query groups by (None: all)."""
    return Query(label, aggs, filter, limit, keys, shift, k, partition, packed)


class Segment:
    """A constructed segment: key columns k0.. over `cards` holding `raw` (sum digit * multiplier), the inputs by name with their values
    as int64 (None for a column that is only filtered on) and the filters by name with their doc masks."""

    def __init__(self, name, cards, raw, inputs, filters=None, double_values=None):
        self.raw = np.ascontiguousarray(raw, dtype=np.int64)
        self.n, self.cards = len(self.raw), list(cards)
        assert self.raw.min() >= 0 and self.raw.max() < int(np.prod(cards)) and self.n <= 140_000
        cols, mult = [], 1
        for i, card in enumerate(cards):
            cols.append(S.Column.from_dict_ids("k%d" % i, (np.arange(card, dtype=np.int64) * 3 - 17).astype(np.int32), (self.raw // mult % card).astype(np.int32)))
            mult *= card
        self.values = {}
        for cname, (column, values) in inputs.items():
            cols.append(column)
            self.values[cname] = values
        self.data = S.SegmentData(name, self.n, cols)
        self.filters = {None: (None, np.ones(self.n, bool))}
        self.filters.update(filters or {})
        self.double_values = double_values or {}

    def raw_keys(self, num_keys):
        return self.raw % int(np.prod(self.cards[:num_keys]))


def irregular_input(rng, n, name="v"):
    """A dictionary INT column whose SUM gathers the signed dictionary value: 50 values over +-2^30 (no value plane: the field would be
    25 bits wider than the dictId)."""
    values = np.unique(np.concatenate([rng.integers(-2 ** 30, 2 ** 30, 48), [-2 ** 30 - 1, 2 ** 30 + 1]])).astype(np.int32)
    ids = rng.integers(0, len(values), n).astype(np.int32)
    return S.Column.from_dict_ids(name, values, ids), values[ids].astype(np.int64)


def affine_input(n, entries, ids, name="a", step=2):
    """A dictionary INT column over an arithmetic progression of `entries` values: the dictId stream is its value plane, log2(entries) bits."""
    values = (np.arange(entries, dtype=np.int64) * step - entries).astype(np.int32)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    return S.Column.from_dict_ids(name, values, ids), values[ids].astype(np.int64), ids.astype(np.int64)


def marker_filters(n, one_doc_at):
    """Column f and three filters over it / the docIds: `nothing` (a dictId no doc holds), `one_doc`, `last_tile` (the last, partial, tile)."""
    ids = (1 + np.arange(n) % 8).astype(np.int32)
    ids[one_doc_at] = 9
    column = S.Column.from_dict_ids("f", np.arange(10, dtype=np.int32) * 11, ids)
    lo = (n - 1) // 2048 * 2048
    docs = np.arange(n)
    return column, ids.astype(np.int64) * 11, lambda f: {
        "nothing": (Q.leaf(Q.Pred.dict_range(f, 0, 1)), np.zeros(n, bool)),
        "one_doc": (Q.leaf(Q.Pred.dict_range(f, 9, 10)), docs == one_doc_at),
        "last_tile": (Q.leaf(Q.Pred.doc_range(lo, n - 1)), docs >= lo),
        "f<=44": (Q.leaf(Q.Pred.dict_range(f, 0, 5)), ids < 5),
        "f>=55": (Q.leaf(Q.Pred.dict_range(f, 5, 10)), ids >= 5),
    }


def standard(name, cards, raw, seed=0, extra=None):
    """Keys plus the inputs most cases share: v (irregular, signed gather), a (affine, 1000 entries: a 10-bit plane field), r (raw INT), f."""
    rng = np.random.default_rng(1000 + seed)
    n = len(raw)
    v = irregular_input(rng, n)
    a = affine_input(n, 1000, rng.integers(0, 1000, n), step=7)
    rvals = rng.integers(-50_000, 50_000, n).astype(np.int32)
    fcol, fvals, filters = marker_filters(n, n // 2)
    inputs = collections.OrderedDict([("v", v), ("a", a[:2]), ("r", (S.Column.raw("r", rvals), rvals.astype(np.int64))), ("f", (fcol, fvals))])
    inputs.update(extra or {})
    seg = Segment(name, cards, raw, inputs)
    seg.filters.update(filters(seg.data.column_index("f")))
    return seg


COUNT, SUM, MIN, MAX = Q.COUNT, Q.SUM, Q.MIN, Q.MAX
COUNT_ONLY = [(COUNT, None)]


def _edge_keys(rng, product, n):
    """Docs on raw keys 0, 4095, 4096 and product - 1, the rest anywhere."""
    raw = rng.integers(0, product, n)
    raw[rng.permutation(n)[:8]] = [0, 4095, 4096, product - 1, 0, 4095, 4096, product - 1]
    return raw


def _boundary_k():
    """The first k >= 5 for which 4096 k - 1, 4096 k and 4096 k + 1 all split into two key cardinalities."""
    k = 5
    while not all(G._factor_pair(4096 * k + d) for d in (-1, 0, 1)):
        k += 1
    return k


def keyspace_case(product, cards, accumulators, shift, k):
    def build():
        rng = np.random.default_rng(product % 100_003)
        seg = standard("keyspace_%d" % product, cards, _edge_keys(rng, product, 6000), seed=product % 97)
        aggs = {0: COUNT_ONLY, 1: [(MAX, "a"), (COUNT, None)], 2: [(SUM, "v"), (MAX, "r"), (COUNT, None)], 3: [(MIN, "v"), (MAX, "v"), (SUM, "r")]}[accumulators]
        packed = {0: 1, 1: 10, 2: 0, 3: 0}[accumulators]
        return seg, [query("%d accumulators" % accumulators, aggs, shift, k, packed), query("%d accumulators, f<=44" % accumulators, aggs, shift, k, packed, filter="f<=44")]
    return build


def doc_count_case(n):
    def build():
        rng = np.random.default_rng(n)
        cards = (300, 400)
        each = standard("docs_%d_each" % n, cards, rng.permutation(120_000)[:n], seed=n)          # one key per doc
        return each, [query("one key per doc, COUNT", COUNT_ONLY, 12, 0, 1), query("one key per doc, SUM(v)", [(SUM, "v"), (COUNT, None)], 12, 0, 0),
                      query("one key per doc, MIN MAX SUM", [(MIN, "r"), (MAX, "a"), (SUM, "v")], 11, 0, 0)]
    return build


def one_key_case(n):
    def build():
        seg = standard("docs_%d_one" % n, (300, 400), np.full(n, 77_777), seed=n + 1)
        return seg, [query("one key, COUNT", COUNT_ONLY, 12, 0, 1), query("one key, SUM(a)", [(SUM, "a")], 12, 0, 10),
                     query("one key, SUM(v) MAX(v)", [(SUM, "v"), (MAX, "v")], 12, 0, 0), query("one key, last tile", [(SUM, "v"), (MIN, "r"), (MAX, "r")], 11, 0, 0, filter="last_tile")]
    return build


def chunk_case(name, cards, lo, hi, k3, k):
    """140 000 docs on the raw keys [lo, hi): more than two 65 536-record chunks in one partition (one level) or coarse partition (two).
    k / k3: log2 of the fine partitions per coarse one with up to two / with three accumulators."""
    def build():
        rng = np.random.default_rng(hi)
        seg = standard(name, cards, rng.integers(lo, hi, 140_000), seed=hi % 89)
        two = [(SUM, "v"), (MIN, "r"), (COUNT, None)]
        three = [(MIN, "v"), (MAX, "v"), (SUM, "r")]
        qs = [query("COUNT", COUNT_ONLY, 12, k, 1), query("SUM(a)", [(SUM, "a")], 12, k, 10), query("two accumulators", two, 12, k, 0),
              query("three accumulators", three, 11, k3, 0)]
        for f in ("nothing", "one_doc", "last_tile"):
            qs += [query("COUNT, " + f, COUNT_ONLY, 12, k, 1, filter=f), query("two accumulators, " + f, two, 12, k, 0, filter=f)]
        return seg, qs
    return build


def packed_width_case(entries_log2, cards, k):
    """One MAX, one MIN and one affine SUM over a dictionary of 2^entries_log2 entries (dictIds 0 and 2^entries_log2 - 1 present): the
    record is packed exactly when entries_log2 + 12 + k <= 32."""
    def build():
        rng = np.random.default_rng(entries_log2 * 10 + k)
        n, entries = 20_000, 1 << entries_log2
        ids = rng.integers(0, entries, n)
        ids[:4] = [0, entries - 1, entries - 1, 0]
        w = affine_input(n, entries, ids, name="w")
        seg = standard("packed_%d_%d" % (entries_log2, k), cards, _edge_keys(rng, int(np.prod(cards)), n), seed=entries_log2, extra={"w": w[:2]})
        bits = entries_log2 if entries_log2 + 12 + k <= 32 else 0
        return seg, [query("MAX(w)", [(MAX, "w")], 12, k, bits), query("MIN(w)", [(MIN, "w"), (COUNT, None)], 12, k, bits), query("SUM(w)", [(SUM, "w")], 12, k, bits),
                     query("MIN(w), f>=55", [(MIN, "w")], 12, k, bits, filter="f>=55")]
    return build


def signedness_case():
    def build():
        rng = np.random.default_rng(31)
        n, product = 9000, 120_000
        raw = rng.integers(0, product, n)
        pool = np.array([-2 ** 31, -1, 0, 2 ** 31 - 1], dtype=np.int64)
        ids = rng.integers(0, 4, n)
        # groups of only the minimum / only the maximum (five docs each: the sums pass 2^32 in magnitude), on both sides of a partition boundary
        for key, d in ((4095, 0), (4096, 3), (product - 1, 0), (0, 3)):
            at = rng.permutation(n)[:5]
            raw[raw == key] = key + 7 if key + 7 < product else key - 7
            raw[at], ids[at] = key, d
        e = S.Column.from_dict_ids("e", pool.astype(np.int32), ids.astype(np.int32))
        rr = pool[ids].astype(np.int32)          # the same values without a dictionary: MIN / MAX then fold the values, not dictIds
        seg = standard("signedness", (300, 400), raw, seed=5, extra={"e": (e, pool[ids]), "re": (S.Column.raw("re", rr), rr.astype(np.int64))})
        return seg, [query("SUM MIN MAX(e)", [(SUM, "e"), (MIN, "e"), (MAX, "e")], 11, 0, 0), query("SUM(e)", [(SUM, "e")], 12, 0, 0),
                     query("MIN(e)", [(MIN, "e")], 12, 0, 2), query("MAX(e)", [(MAX, "e"), (COUNT, None)], 12, 0, 2),
                     query("SUM MIN MAX(raw)", [(SUM, "re"), (MIN, "re"), (MAX, "re")], 11, 0, 0), query("MIN(raw) MAX(raw)", [(MIN, "re"), (MAX, "re")], 12, 0, 0)]
    return build


def accumulators_case():
    def build():
        rng = np.random.default_rng(34)
        seg = standard("accumulators", (300, 400), _edge_keys(rng, 120_000, 30_000), seed=34)
        return seg, [query("three: MIN MAX SUM(v)", [(MIN, "v"), (MAX, "v"), (SUM, "v"), (Q.COUNT, None)], 11, 0, 0),
                     query("four", [(MIN, "v"), (MAX, "v"), (SUM, "v"), (SUM, "r")], 11, 0, 0, partition=False),
                     query("three: over three columns", [(SUM, "a"), (MAX, "r"), (MIN, "v")], 11, 0, 0)]
    return build


def histogram_cache_case():
    """The same keys under two filters back to back (the second reads the cached unfiltered histogram), then with three accumulators
    (another shift: another cache entry), then the first again."""
    def build():
        rng = np.random.default_rng(35)
        seg = standard("histogram_cache", (300, 400), np.minimum(rng.integers(0, 120_000, 50_000), rng.integers(0, 120_000, 50_000)), seed=35)
        two, three = [(SUM, "v"), (MAX, "r")], [(SUM, "v"), (MAX, "r"), (MIN, "a")]
        return seg, [query("two accumulators, f<=44", two, 12, 0, 0, filter="f<=44"), query("two accumulators, f>=55", two, 12, 0, 0, filter="f>=55"),
                     query("three accumulators, f<=44", three, 11, 0, 0, filter="f<=44"), query("three accumulators", three, 11, 0, 0),
                     query("two accumulators", two, 12, 0, 0), query("two accumulators, f<=44 again", two, 12, 0, 0, filter="f<=44")]
    return build


def context_reuse_case():
    """One open segment: a two-level query, a one-level query, a direct-table query (a DOUBLE sum), the first again."""
    def build():
        rng = np.random.default_rng(36)
        n = 40_000
        raw = _edge_keys(rng, 300 * 400 * 30, n)
        halves = rng.integers(-2000, 2000, n)
        d = S.Column.dict_encoded_typed("d", halves * 0.5)
        seg = standard("context_reuse", (300, 400, 30), raw, seed=36, extra={"d": (d, None)})
        seg.double_values["d"] = halves * 0.5
        two_level = query("two-level", [(SUM, "v"), (COUNT, None)], 12, 1, 0)
        return seg, [two_level, query("one-level", [(SUM, "v"), (COUNT, None)], 12, 0, 0, keys=2), query("direct table: SUM(d)", [(SUM, "d")], 12, 1, 0, partition=False),
                     two_level._replace(label="two-level again")]
    return build


def limits_case(name, cards, k):
    def build():
        rng = np.random.default_rng(37 + k)
        n, product = 12_000, int(np.prod(cards))
        pool = np.unique(np.concatenate([rng.integers(0, product, 1500), [0, 4095, 4096, product - 1]]))
        seg = standard(name, cards, pool[rng.integers(0, len(pool), n)], seed=37 + k)
        present = len(np.unique(seg.raw))
        present_f = len(np.unique(seg.raw[seg.filters["f<=44"][1]]))
        aggs = [(COUNT, None), (SUM, "v"), (MIN, "r")]
        return seg, [query("limit %+d" % d, aggs, 12, k, 0, limit=present + d) for d in (-1, 0, 1)] + [query("limit 1", COUNT_ONLY, 12, k, 1, limit=1)] + \
            [query("f<=44, limit %+d" % d, aggs, 12, k, 0, filter="f<=44", limit=present_f + d) for d in (-1, 0, 1)]
    return build


def wide_case():
    def build():
        rng = np.random.default_rng(38)
        cards = (4099, 4099, 2)
        product = int(np.prod(cards))
        seg = standard("wide", cards, _edge_keys(rng, product, 20_000), seed=38)
        return seg, [query("COUNT", COUNT_ONLY, 12, 5, 1), query("SUM(a)", [(SUM, "a")], 12, 5, 10), query("SUM(v) MAX(r)", [(SUM, "v"), (MAX, "r")], 12, 5, 0),
                     query("MIN MAX SUM(v)", [(MIN, "v"), (MAX, "v"), (SUM, "v")], 11, 6, 0)]
    return build


BK = _boundary_k()
CASES = collections.OrderedDict()
# (10 001 keys x COUNT alone are an 80 KB table: that one fits the LDS of group_private_kernel and is not partitioned; one accumulator is 160 KB)
for _product in (10_001, 4096 * BK - 1, 4096 * BK, 4096 * BK + 1):
    _a, _b = G._factor_pair(_product)
    for _acc in ((1, 2, 3) if _product == 10_001 else (0, 2, 3)):
        CASES["keyspace %d, %d accumulators" % (_product, _acc)] = (keyspace_case(_product, (_b, _a), _acc, 11 if _acc == 3 else 12, 0), None)
# 512 partitions in one level, and the first two-level key space: at shift 12 (2^21) and one bit lower with three accumulators (shift 11)
CASES["keyspace 2^21 = 2048 x 1024: one level"] = (keyspace_case(1 << 21, (2048, 1024), 2, 12, 0), None)
CASES["keyspace 2^21 + 1 = 3 x 699051: two levels"] = (keyspace_case((1 << 21) + 1, (3, 699_051), 2, 12, 1), None)
CASES["keyspace 2^21 COUNT: one level"] = (keyspace_case(1 << 21, (2048, 1024), 0, 12, 0), None)
CASES["keyspace 2^21 + 1 COUNT: two levels"] = (keyspace_case((1 << 21) + 1, (699_051, 3), 0, 12, 1), None)
CASES["keyspace 2^20 = 1024 x 1024, three accumulators: one level"] = (keyspace_case(1 << 20, (1024, 1024), 3, 11, 0), None)
CASES["keyspace 2^20 + 1 = 17 x 61681, three accumulators: two levels"] = (keyspace_case((1 << 20) + 1, (17, 61_681), 3, 11, 1), None)
for _n in (1, 2047, 2049, 8191, 8193, 65_535, 65_537):
    CASES["%d docs, one key per doc" % _n] = (doc_count_case(_n), None)
    CASES["%d docs, one key" % _n] = (one_key_case(_n), None)
# 300 x 400: raw keys 4096 .. 8191 are partition 1 at shift 12 and partitions 2 and 3 at shift 11
CASES["chunks: one partition of three work items"] = (chunk_case("chunk_one_level", (300, 400), 4096, 8192, 0, 0), None)
# 3 x 699051 (two fine partitions of 4096 keys per coarse one): raw keys 8192 .. 12287 are ONE fine partition of coarse partition 1
CASES["chunks: one coarse partition, one fine partition"] = (chunk_case("chunk_two_level_one_fine", (3, 699_051), 8192, 12_288, 2, 1), None)
# 3000 x 2900 = 8.7 M keys (eight fine partitions per coarse one, sixteen at shift 11): raw keys 32768 .. 65535 are ALL of coarse partition 1
CASES["chunks: one coarse partition, all eight fine partitions"] = (chunk_case("chunk_two_level_all_fine", (3000, 2900), 32_768, 65_536, 4, 3), None)
UNPACKED = {"PINOT_GPU_PARTITION_PACKED": "0"}
CASES["packed width 20 + 12 = 32: packed"] = (packed_width_case(20, (300, 400), 0), UNPACKED)
CASES["packed width 21 + 12 = 33: not packed"] = (packed_width_case(21, (300, 400), 0), UNPACKED)
CASES["packed width 19 + 13 = 32, two levels: packed"] = (packed_width_case(19, (3, 699_051), 1), UNPACKED)
CASES["packed width 20 + 13 = 33, two levels: not packed"] = (packed_width_case(20, (3, 699_051), 1), UNPACKED)
CASES["signedness and identities"] = (signedness_case(), UNPACKED)
CASES["three and four accumulators"] = (accumulators_case(), None)
CASES["histogram cache"] = (histogram_cache_case(), {"PINOT_GPU_PARTITION_STATS_CACHE": "0"})
CASES["context reuse"] = (context_reuse_case(), None)
CASES["limits, one level"] = (limits_case("limits_one_level", (300, 400), 0), None)
CASES["limits, two levels"] = (limits_case("limits_two_level", (3000, 2900), 3), None)
CASES["wide: above 2^24, three keys"] = (wide_case(), None)

_PLANNED = {}       # case name -> (segment, queries, specs)
_BUILT = {}         # case name -> (segment, queries, specs, oracle results, numpy group-bys)


def numpy_group_by(seg, q, num_keys):
    """The query by plain numpy over the raw keys: {raw key: [(count, value) per aggregation]}; under a binding limit the first keys in
    docId order (group_map_cases.admitted_keys)."""
    raw, mask = seg.raw_keys(num_keys), seg.filters[q.filter][1]
    keys, inverse = np.unique(raw[mask], return_inverse=True)
    counts = np.bincount(inverse, minlength=len(keys))
    columns = []
    for f, cname in q.aggs:
        if f == COUNT:
            columns.append(counts)
            continue
        values = (seg.double_values[cname] if cname in seg.double_values else seg.values[cname])[mask]
        if f == SUM:
            out = np.zeros(len(keys), dtype=values.dtype)
            np.add.at(out, inverse, values)
        else:
            out = np.full(len(keys), values.max() if f == MIN else values.min(), dtype=values.dtype) if len(keys) else np.zeros(0, values.dtype)
            (np.minimum if f == MIN else np.maximum).at(out, inverse, values)
        columns.append(out)
    limit = q.limit if q.limit > 0 else 100_000
    admitted = GM.admitted_keys(raw, mask, limit) if len(keys) > limit else None
    return {int(key): [(int(counts[i]), col[i].item()) for col in columns] for i, key in enumerate(keys) if admitted is None or int(key) in admitted}


def planned(name):
    if name not in _PLANNED:
        seg, queries = CASES[name][0]()
        ci = seg.data.column_index
        specs = [Q.QuerySpec([(f, -1 if c is None else ci(c)) for f, c in q.aggs], filter=seg.filters[q.filter][0],
                             group_by=[ci("k%d" % i) for i in range(q.keys or len(seg.cards))], num_groups_limit=q.limit) for q in queries]
        _PLANNED[name] = (seg, queries, specs)
    return _PLANNED[name]


def built(name):
    """The case with its references, computed once and shared by both grid sizes."""
    if name not in _BUILT:
        seg, queries, specs = planned(name)
        _BUILT[name] = (seg, queries, specs, [oracle.execute(seg.data, spec) for spec in specs], [numpy_group_by(seg, q, q.keys or len(seg.cards)) for q in queries])
    return _BUILT[name]


def check_against_numpy(got, q, model):
    assert list(got.groups) == sorted(model), "rows: %d, numpy %d" % (len(got.groups), len(model))
    for key, row in model.items():
        for i, ((f, _), (count, value)) in enumerate(zip(q.aggs, row)):
            v = got.groups[key][i]
            assert v.count == count, "group %d agg %d: count %d, numpy %d" % (key, i, v.count, count)
            if f == SUM and isinstance(value, int):
                assert v.sum_i64 == value and v.sum_exact, "group %d agg %d: sum %d, numpy %d" % (key, i, v.sum_i64, value)
            elif f == SUM:
                assert v.sum == value, "group %d agg %d: sum %r, numpy %r" % (key, i, v.sum, value)
            elif f in (MIN, MAX):
                assert (v.min if f == MIN else v.max) == float(value), "group %d agg %d: %r, numpy %r" % (key, i, v.min if f == MIN else v.max, value)


def announce_case(engine, name):
    """The child's run: every query of the case, announced on stderr in front of the engine's own plan line."""
    seg, queries, specs = planned(name)
    with engine.open(seg.data) as g:
        for q, spec in zip(queries, specs):
            sys.stderr.write("edge-case: %s | %s\n" % (name, q.label))
            sys.stderr.flush()
            g.execute(spec)


def run_case(engine, name):
    """Every query of the case, in order, on one open segment: against the oracle, numpy and the kernel the query is named for."""
    seg, queries, specs, wants, models = built(name)
    results = []
    with engine.open(seg.data) as g:
        for q, spec, want, model in zip(queries, specs, wants, models):
            got = g.execute(spec)
            try:
                H.assert_results_equal(got, want, check_stats=True)
                assert got.num_groups_limit_reached == want.num_groups_limit_reached and got.group_id_upper_bound == want.group_id_upper_bound
                check_against_numpy(got, q, model)
                assert (got.dominant_kernel == G.SCATTER_KERNEL) == q.partition, "partitioned: %r" % q.partition
            except AssertionError as e:
                raise AssertionError("%s | %s [%s]: %s" % (name, q.label, got.dominant_kernel, e)) from e
            results.append(got)
    return results


@pytest.fixture(params=[None, "1"], ids=["whole-device", "one-cu"])
def forced(engine, request):
    engine.reinit(**dict({k: None for k in SWITCHES}, PINOT_GPU_GROUP_PARTITION="force", PINOT_GPU_TEST_CUS=request.param))
    try:
        yield engine
    finally:
        engine.reinit(**{k: None for k in SWITCHES})


@pytest.mark.parametrize("name", list(CASES))
def test_pinned_case(forced, name):
    first = run_case(forced, name)
    seg, queries, _, _, _ = built(name)
    if name == "context reuse":
        same_results(first[-1], first[0])
    other_side = CASES[name][1]
    if other_side:
        # once more with the switch flipped (unpacked records; no histogram cache): the same tables
        forced.reinit(**other_side)
        again = run_case(forced, name)
        for q, a, b in zip(queries, first, again):
            try:
                same_results(b, a)
            except AssertionError as e:
                raise AssertionError("%s | %s under %r: %s" % (name, q.label, other_side, e)) from e


def test_the_plan_arithmetic_the_cases_are_named_for():
    """The stated plans against the generator's mirror of the planner (itself pinned in tests/test_fuzz_group_cases_cpu.py)."""
    for name in CASES:
        seg, queries, specs = planned(name)
        for q, spec in zip(queries, specs):
            product = int(np.prod(seg.cards[: len(spec.group_by)]))
            accumulators = len({(c, f) for f, c in q.aggs if f != COUNT})
            shift, _, k, _ = G.plan(product, accumulators)
            assert (q.shift, q.k) == (shift, k), "%s | %s: named for shift %d, 2^%d; the arithmetic gives shift %d, 2^%d" % (name, q.label, q.shift, q.k, shift, k)


PLAN_LINE = re.compile(r"group-by plan: product (\d+), fine partitions (\d+) \(shift (\d+)\), 2\^(\d+) per coarse -> (\d+) scatter partitions; partition (\d) .* packed_bits (\d+)\)")


def test_every_case_took_the_plan_it_is_named_for():
    """A fresh child (the trace switch is read once per process) runs every case under the forced routing with PINOT_GPU_PARTITION_TRACE=1; its
    "group-by plan:" lines must show the shift, the level count, the partition decision and the packed width each query is named for."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PINOT_GPU_PARTITION_TRACE="1", PINOT_GPU_GROUP_PARTITION="force")
    for k in list(env):
        if k.startswith("PINOT_GPU_") and k not in ("PINOT_GPU_LIB", "PINOT_GPU_PARTITION_TRACE", "PINOT_GPU_GROUP_PARTITION"):
            del env[k]
    proc = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = proc.stderr.decode()
    assert proc.returncode == 0 and b"edge cases done" in proc.stdout, err[-3000:]
    plans, current = {}, None
    for line in err.splitlines():
        if line.startswith("edge-case: "):
            current = line[len("edge-case: "):]
            plans[current] = []
        elif current is not None and line.startswith("group-by plan:"):
            m = PLAN_LINE.match(line)
            assert m, "unreadable plan line: " + line
            plans[current].append(tuple(int(x) for x in m.groups()))
    checked = 0
    for name in CASES:
        seg, queries, specs = planned(name)
        for q, spec in zip(queries, specs):
            lines = plans.get("%s | %s" % (name, q.label))
            assert lines, "%s | %s: no plan line" % (name, q.label)
            product = int(np.prod(seg.cards[: len(spec.group_by)]))
            for got_product, fine, shift, k, scatter, partition, packed in lines:
                at = "%s | %s: %r" % (name, q.label, lines)
                assert got_product == product and shift == q.shift and k == q.k and bool(partition) == q.partition, at
                assert fine == (product + (1 << shift) - 1) >> shift and scatter == (fine + (1 << k) - 1) >> k and scatter <= 512, at
                assert packed == (q.packed if q.partition else 0), at
            checked += 1
    assert checked >= 150


if __name__ == "__main__":
    # the child of test_every_case_took_the_plan_it_is_named_for: every case once, announced on stderr between the engine's plan lines
    from pinot_amd.engine import Engine
    child_engine = Engine(device_id=0)
    for case_name in CASES:
        announce_case(child_engine, case_name)
    print("edge cases done: %d" % len(CASES))
