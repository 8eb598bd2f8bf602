"""Randomised GROUP BY segments and queries over key spaces ABOVE the array-based threshold (product of the key cardinalities > 10 000): the
partitioned group-by (pg_group_partition.h, run_partitioned_group_by), the direct HBM table of group_private_kernel / scan_group_kernel and
compact_map_groups.  Built on tests/fuzz_cases.py: its Col / Segment / FuzzQuery, its filter trees and its EXACT MODEL (`expected`,
`check_result`) are used as they are; this module only draws other segments and queries and says, per query, which plan the engine's
planner arithmetic gives it (`describe`).  Shared by tests/test_fuzz_group_cases_cpu.py (oracle vs. model, class coverage) and
tests/test_gpu_fuzz_groups.py (device vs. oracle and model under every routing).  Nothing here needs a GPU or the oracle.  Deterministic in
(seed); PINOT_FUZZ_SEED_BASE shifts every seed.

Segments: `num_docs` around the 2048-doc tile, the 8192-doc scatter round and the 65 536-record chunk (SIZES), never above 140 000 -- the
partitioned path engages below 2^22 docs only under PINOT_GPU_GROUP_PARTITION=force.  Two or three key columns whose cardinalities are
drawn so that their product falls into a class (TARGETS): `lds` controls over two small keys, `one-level` (10 001 .. 512 * 2^shift; the
4096-key partition boundaries -1 / 0 / +1; exactly 2^20 and 2^21), `two-level` (2^20 + 1 and 2^21 + 1, then up to 9 M: 2, 4 and 8 fine
partitions per coarse one), `wide` (three keys, product just above 2^25, the third key's multiplier above 2^24: the 32-bit key multiply).
Key kinds: dictionary INT at natural and forced width, dictionary LONG / FLOAT / DOUBLE (the digit is the dictId), a raw INT key through
its offset image.  Key distributions (DISTRIBUTIONS): uniform and min-of-two-uniforms over a pool of distinct keys, every doc in one
partition, every doc on one key, one heavy key plus docs that sit alone in partitions of their own.  Raw key 0 and raw key product - 1 are
always present (with one doc the last key only); a LONG / FLOAT / DOUBLE key column has every dictId present, so a few pinned docs lie
outside "one partition" / "one key".
Aggregation inputs: dictionary INT with an affine dictionary (SUM reads a value-plane field, here the dictId stream itself), an
irregular one (SUM gathers the signed dictionary value), the INT edges -2^31, -1, 0, 1, 2^31-1; sum-safe dictionary LONG; dictionary
DOUBLE, benign and ill-conditioned; raw INT.  1-5 aggregations in fixed shapes (QUERY_SHAPES) so that every record format occurs in
every segment: COUNT alone, one unsigned input, one signed input, two and three accumulators, MIN + MAX + SUM of one column, more than
three accumulators, a LONG / DOUBLE sum, free draws.  Null vectors and null handling as in fuzz_cases; filters from fuzz_cases._make_tree
plus three fixed kinds (FIXED_FILTERS): matches nothing, exactly one doc, only the docs of the last tile; num_groups_limit out of 0, 5,
200, the number of groups present and one less.

What is NOT generated, and why:
  * everything fuzz_cases keeps out of a GROUP BY: SUM / AVG over a LONG column that is not sum-safe (declined: could overflow int64),
    a nullable raw key column (declined under null handling), MIN / MAX over NaN under null handling and MAX over a dictionary that
    holds NaN (no NaN in any pool here), two-zero dictionaries (np.unique merges them), hashed holders (products stay below 2^31);
  * raw LONG / FLOAT / DOUBLE columns, as keys, inputs or filter columns: group_typed_direct_kernel and the rank images have
    tests/fuzz_cases.py and tests/rank_key_cases.py; without them every filter leaf is lane-private, which the partitioned path needs;
  * more than 4 000 distinct keys per segment: a result row costs the Python side more than the device; one key
    per doc at the chunk boundaries is pinned in tests/test_gpu_group_partition_edges.py;
  * SUM over an irregular INT dictionary wide enough for a materialised value plane (want_value_plane, pg_engine.hip): the plane is
    built asynchronously, so whether a query packs its records would depend on timing; irregular dictionaries here span ~2^31 over at
    most 4 000 entries and always gather.
Two of the committed seeds' queries are still declined on the device ("more than 8 filter leaves"): under null handling the filter is
rewritten with IS NOT NULL leaves of its nullable columns, which a tree of up to eight leaves can push over the cap; static_decline
below counts the tree as written.  The GPU test caps declines at 10 %."""
import numpy as np

import fuzz_cases as F
from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S

SEED_BASE = F.SEED_BASE
SEEDS = list(range(24))
SIZES = [1, 2047, 2049, 8191, 8192, 8193, 20_011, 65_535, 65_537, 70_001, 131_073, 140_000]

# the planner's arithmetic, mirrored (pg_group_plan.h partition_plan, the limits of pg_device.h; tests/test_group_plan_cpu.py holds `plan` and
# the four partition limits below against the header's stand-alone check)
ARRAY_BASED_THRESHOLD = F.ARRAY_BASED_THRESHOLD   # pg_engine.hip bind_group_keys  map_based = product > 10000 || first_appearance
DEFAULT_GROUPS_LIMIT = F.DEFAULT_GROUPS_LIMIT     # pg_engine.hip groups_limit     num_groups_limit > 0 ? num_groups_limit : 100000
MAX_PARTITIONS = 512                              # pg_device.h         kMaxPartitions
MAX_PARTITION_AGGS = 3                            # pg_device.h         kMaxPartitionAggs
MAX_FINE_PER_COARSE = 1024                        # pg_device.h         kMaxFinePerCoarse
REPARTITION_CHUNK = 1 << 16                       # pg_device.h         kRepartitionChunk
SCATTER_ROUND_DOCS = 8192                         # pg_group_partition.h kScatterDocsPerRound
TILE_DOCS = 2048
WIDE_KEYS = 1 << 24                               # pg_engine.hip bind_group_aggs  gp.wide_keys = product > (1ll << 24)
SCATTER_KERNEL = "group_partition_scatter_kernel"


def plan(product, accumulators):
    """(shift, fine partitions, log2_fine_per_coarse, scatter partitions) of a key space: entry bytes = 4 + 8 x accumulators; shift 12
    when the entry is at most 20 bytes, else 11; one level up to 512 partitions (pg_group_plan.h partition_plan)."""
    entry_bytes = 4 + 8 * accumulators
    shift = 12 if entry_bytes <= 20 else 11
    fine = (product + (1 << shift) - 1) >> shift
    k = 0
    while ((fine + (1 << k) - 1) >> k) > MAX_PARTITIONS:
        k += 1
    return shift, fine, k, (fine + (1 << k) - 1) >> k


# key-space target of every seed (the doc count is SIZES[seed % 12]): every class meets small and large segments
TARGETS = ["one", "two1", "one_edge", "two2", "one", "two3", "one_top21", "two_first21", "wide", "one", "two1", "one",
           "two2", "one_top20", "two_first20", "one", "two3", "one_edge", "wide", "one", "two1", "two2", "one_edge", "two3"]
RANGES = {"one": (10_001, 1 << 20), "two1": ((1 << 21) + 1, 1 << 22), "two2": ((1 << 22) + 1, 1 << 23), "two3": ((1 << 23) + 1, 9_000_000)}
EXACT = {"one_top21": (2048, 1024), "one_top20": (1024, 1024), "two_first21": (3, 699_051), "two_first20": (17, 61_681)}
DISTRIBUTIONS = ["uniform", "min2", "one_partition", "one_key", "sparse"]
FIXED_FILTERS = ["nothing", "one_doc", "last_tile"]
QUERY_SHAPES = ["count", "unsigned1", "signed1", "two", "three", "min_max_sum", "many", "wide_sum", "free", "free", "lds", "lds"]
SMALL_KEY_KINDS = ["dict_int", "dict_int_forced", F.DICT_LONG, F.DICT_FLOAT, F.DICT_DOUBLE, F.RAW_INT]


class GroupSegment(F.Segment):
    """F.Segment plus: the key columns (`keys`, column indexes in multiplier order), the two small keys of the lds controls
    (`small_keys`), the key-space target and distribution, every key column's digit per doc (`digits`: dictId, or value - min of the raw
    key) and the aggregation inputs by role (`roles`)."""

    def __init__(self, seed, n, cols):
        self.seed, self.n, self.cols = seed, n, cols
        self.data = S.SegmentData("fuzzg%d" % seed, n, [c.column for c in cols])
        self.keys, self.small_keys, self.target, self.distribution, self.digits, self.roles = [], [], "", "", {}, {}


# ------------------------------------------------------------------------------------------------------------------------------------
# segments
# ------------------------------------------------------------------------------------------------------------------------------------
def _factor_pair(m):
    """(a, b), a * b == m, 2 <= a <= b, a as large as it gets below 4096; None for a prime."""
    for a in range(min(4095, int(m ** 0.5)), 1, -1):
        if m % a == 0:
            return a, m // a
    return None


def _draw_cards(rng, target, n):
    """The key cardinalities (multiplier order) and the kinds of the keys behind the first."""
    typed_ok = n >= 64                      # a typed dictionary holds what occurs: every dictId needs a doc
    def small_kind():
        return F._pick(rng, SMALL_KEY_KINDS if typed_ok else SMALL_KEY_KINDS[:2])
    if target == "wide":
        return [4099 + int(rng.integers(0, 6)), 4099 + int(rng.integers(0, 6)), 2], ["dict_int", F._pick(rng, ["dict_int", "dict_int_forced"]), small_kind()]
    if target in EXACT:
        cards = list(EXACT[target])
        if rng.integers(0, 2):
            cards.reverse()
        return cards, ["dict_int", F._pick(rng, ["dict_int", "dict_int_forced"])]
    if target == "one_edge":
        while True:
            m = 4096 * int(rng.integers(3, 200)) + int(rng.integers(-1, 2))
            pair = _factor_pair(m)
            if pair:
                return [pair[1], pair[0]], ["dict_int", F._pick(rng, ["dict_int", "dict_int_forced"])]
    lo, hi = RANGES[target]
    while True:
        kinds = ["dict_int", small_kind()] + ([small_kind()] if rng.integers(0, 2) else [])
        rest = [int(rng.integers(2, 41)) if k not in ("dict_int", "dict_int_forced") else int(rng.choice([2, 3, 7, 64, 1000, 3000])) for k in kinds[1:]]
        t = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
        c0 = max(2, t // int(np.prod(rest)))
        if lo <= c0 * int(np.prod(rest)) <= hi:
            return [c0] + rest, kinds


def _draw_raw_keys(rng, dist, n, product):
    """The raw key of every doc (int64) for one distribution; see the module docstring."""
    if dist in ("uniform", "min2"):
        pool = np.unique(rng.integers(0, product, min(n, int(rng.choice([50, 1000, 4000])))))
        a = rng.integers(0, len(pool), n)
        return pool[np.minimum(a, rng.integers(0, len(pool), n)) if dist == "min2" else a]
    partitions = (product + 4095) // 4096
    if dist == "one_partition":             # a 2048-key window of one 4096-key range: one partition at either shift
        base = int(rng.integers(0, partitions)) * 4096
        pool = np.unique(np.minimum(base + rng.integers(0, 2048, 300), product - 1))
        return pool[rng.integers(0, len(pool), n)]
    raw = np.full(n, int(rng.integers(0, product)), dtype=np.int64)
    if dist == "sparse":                    # one heavy key; the other docs alone in partitions of their own
        m = int(min(n // 4, partitions, 600))
        parts = rng.choice(partitions, m, replace=False).astype(np.int64)
        raw[rng.choice(n, m, replace=False)] = np.minimum(parts * 4096 + rng.integers(0, 4096, m), product - 1)
    return raw


def _widen(col, ids, bits):
    """Pack a dictionary column's forward index at `bits` > its natural width (tests/test_gpu_fuzz.py's forced widths)."""
    host = S.load_host_library()
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    col.bits = bits
    col.fwd = np.zeros(int(host.ph_fixedbit_size(len(ids), bits)), dtype=np.uint8)
    host.ph_fixedbit_pack(S._i32p(ids), len(ids), bits, S._u8p(col.fwd), 2)


def _dict_int(rng, name, values, ids, forced):
    values = np.ascontiguousarray(values, dtype=np.int32)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    col = S.Column.from_dict_ids(name, values, ids)
    if forced and col.bits < 31:
        _widen(col, ids, int(rng.integers(col.bits + 1, 32)))
    return F.Col(name, F.DICT_INT, values[ids], col, ids=ids, dict_values=values)


def _key_column(rng, name, kind, card, digits):
    if kind in ("dict_int", "dict_int_forced"):
        return _dict_int(rng, name, np.arange(card, dtype=np.int64) * 3 - 17, digits, kind == "dict_int_forced")
    if kind == F.RAW_INT:
        values = (int(rng.integers(-1000, 1000)) + digits).astype(np.int32)
        return F.Col(name, F.RAW_INT, values, S.Column.raw(name, values))
    pool = {F.DICT_LONG: int(rng.choice([-1, 1])) * (2 ** 40 - 5000) + np.arange(card, dtype=np.int64) * 7,
            F.DICT_FLOAT: (np.arange(card) * 0.5 - 3.0).astype(np.float32),
            F.DICT_DOUBLE: np.arange(card) * 0.1 - 1.0}[kind]
    c = F._typed_dict(name, kind, pool[digits], pool="benign" if kind != F.DICT_LONG else None)
    assert np.array_equal(c.ids, digits), "a typed key column whose dictIds are not its digits"
    return c


def _plane_bits(values):
    """compute_plane_shape (pg_engine.hip): the width of the gcd-scaled offset field of an INT dictionary."""
    v = np.asarray(values, dtype=np.int64)
    g = int(np.gcd.reduce(v - v[0])) or 1
    top, w = int(v[-1] - v[0]) // g, 1
    while w < 32 and (top >> w) != 0:
        w += 1
    return w, top == len(v) - 1 and w < 32


def _input_columns(rng, n):
    """The aggregation inputs, by role."""
    out = {}
    card = int(rng.choice([2, 100, 5000]))
    out["affine"] = _dict_int(rng, "affine", np.arange(card, dtype=np.int64) * int(rng.integers(1, 9)) + int(rng.integers(-1000, 1000)),
                              rng.integers(0, card, n), bool(rng.integers(0, 2)))
    card = int(rng.choice([3, 60, 4000]))
    values = np.sort(rng.permutation(np.unique(rng.integers(-2 ** 30, 2 ** 30, 2 * card)))[:card])
    card = len(values)
    values[0], values[-1] = -2 ** 30 - 1, 2 ** 30 + 1       # (the span alone puts the plane field 19 bits above the dictId: no plane, the SUM gathers)
    out["irregular"] = _dict_int(rng, "irregular", values, rng.integers(0, card, n), False)
    pool = np.array(F.INT_EDGES + [int(x) for x in rng.integers(-2 ** 31, 2 ** 31, int(rng.integers(1, 25)))], dtype=np.int32)
    out["edges"] = F._typed_dict("edges", F.DICT_INT, F._draw(rng, pool, n))
    for role in ("affine", "irregular", "edges"):
        bits, is_fwd = _plane_bits(out[role].dict_values)
        # what describe() relies on: an arithmetic progression (the plane is the dictId stream), or no value plane at all (want_value_plane)
        assert (is_fwd or role != "affine") and (is_fwd or (bits - out[role].column.bits > 8 and out[role].cardinality <= 8192)), role
    pool = np.array(F.LONG_SAFE_EDGES + [int(x) for x in rng.integers(-2 ** 40, 2 ** 40, int(rng.integers(1, 20)))], dtype=np.int64)
    out["long"] = F._typed_dict("long", F.DICT_LONG, F._draw(rng, pool, n), sum_safe=True)
    for role in ("benign", "ill"):
        out[role] = F._typed_dict(role, F.DICT_DOUBLE, F._draw(rng, F._fp_pool(rng, np.float64, role), n).astype(np.float64), pool=role)
    pool = (np.arange(41) - 20) * int(rng.integers(1, 4)) if rng.integers(0, 2) else np.array(F.INT_EDGES + [int(x) for x in rng.integers(-2 ** 31, 2 ** 31, 9)])
    drawn = F._draw(rng, pool.astype(np.int32), n)
    out["raw"] = F.Col("raw", F.RAW_INT, drawn, S.Column.raw("raw", drawn))
    return out


def _add_nulls(rng, c, n):
    style = int(rng.integers(0, 6))
    mask = None
    if style == 1:
        mask = rng.random(n) < 0.01
    elif style == 2:
        mask = rng.random(n) < 0.7
    elif style == 3:
        mask = np.zeros(n, bool)
        mask[n // 3: n // 3 + max(1, n // 5)] = True
    if mask is not None and mask.any():
        c.column.with_nulls(mask)
        c.nulls = mask


def make_segment(seed):
    rng = np.random.default_rng(55_000 + SEED_BASE + seed)
    n = SIZES[seed % len(SIZES)]
    target, dist = TARGETS[seed % len(TARGETS)], DISTRIBUTIONS[seed % len(DISTRIBUTIONS)]
    cards, kinds = _draw_cards(rng, target, n)
    product = int(np.prod(cards))
    raw = _draw_raw_keys(rng, dist, n, product).astype(np.int64)
    mults = [int(np.prod(cards[:i])) for i in range(len(cards))]
    # the pinned docs: the last and the first raw key, then every dictId of a typed key column
    pins = [product - 1, 0]
    spots = rng.permutation(n)
    for card, kind, mult in zip(cards, kinds, mults):
        if kind in (F.DICT_LONG, F.DICT_FLOAT, F.DICT_DOUBLE):
            for d in range(card):
                base = int(raw[spots[len(pins) % n]])
                pins.append(base - (base // mult % card) * mult + d * mult)
    for i, key in enumerate(pins[:n]):
        raw[spots[i]] = key
    cols, digits = [], {}
    for i, (card, kind, mult) in enumerate(zip(cards, kinds, mults)):
        digits[i] = (raw // mult % card).astype(np.int64)
        cols.append(_key_column(rng, "k%d" % i, kind, card, digits[i]))
        assert cols[-1].key_scale()[2] == card or n < 2, "key column k%d: cardinality %d, drawn %d" % (i, cols[-1].key_scale()[2], card)
    small = []
    for j, card in enumerate((int(rng.choice([2, 7, 50])), int(rng.choice([3, 40, 190])))):
        small.append(len(cols))
        digits[len(cols)] = rng.integers(0, card, n).astype(np.int64)
        cols.append(_dict_int(rng, "s%d" % j, np.arange(card, dtype=np.int64) * 5 - 7, digits[len(cols)], bool(rng.integers(0, 2))))
    roles = {}
    for role, c in _input_columns(rng, n).items():
        roles[role] = len(cols)
        cols.append(c)
    # null value vectors: on the aggregation inputs, and on one dictionary key of some segments (never on a raw key)
    for role, ci in roles.items():
        _add_nulls(rng, cols[ci], n)
    if len(cards) > 1 and cols[1].is_dict and rng.integers(0, 3) == 0:
        _add_nulls(rng, cols[1], n)
    seg = GroupSegment(seed, n, cols)
    seg.keys, seg.small_keys, seg.target, seg.distribution, seg.digits, seg.roles = list(range(len(cards))), small, target, dist, digits, roles
    return seg


# ------------------------------------------------------------------------------------------------------------------------------------
# what the planner makes of a query
# ------------------------------------------------------------------------------------------------------------------------------------
class GroupInfo:
    """One query's plan by the engine's arithmetic.  `product`: of the key cardinalities, a nullable key under null handling counting its
    NULL digit; `accumulators`: distinct (column, SUM | MIN | MAX) pairs of the launch that decides the groups (under null handling the
    aggregations over nullable columns run in lanes of their own: execute_null_handling, pg_engine.hip); `klass`: lds / one-level /
    two-level / wide; `shift`, `log2_fine_per_coarse`; `map_based`; `int32_inputs`; `packed_bits` (0: separate key / value columns);
    `partitionable`: what PINOT_GPU_GROUP_PARTITION=force partitions (choose_group_route's use_partition, with every filter leaf lane-private
    as they all are here).  `lane_plans`: (partitionable, log2_fine_per_coarse) of every launch the query is answered from -- one, or under
    null handling the base lane and one lane per nullable aggregated column; Result.dominant_kernel is the kernel of the lane whose
    kernel ran longest, a measured time, so it can be foretold only where the lanes agree."""

    def labels(self):
        """The classes of tests/test_fuzz_group_cases_cpu.py's coverage that this query stands for."""
        out = set()
        if len(self.accumulators) > MAX_PARTITION_AGGS:
            out.add("more than 3 accumulators")
        if not self.int32_inputs:
            out.add("non-INT32 input")
        if self.klass == "lds" and not self.map_based:
            out.add("lds")
        if not self.partitionable:
            return out
        level = "two-level" if self.log2_fine_per_coarse > 0 else "one-level"
        if self.klass == "wide":
            out.add("wide")
        if level == "two-level":
            out.add("two-level packed" if self.packed_bits else "two-level unpacked")
            out.add("fine per coarse 2^%d" % self.log2_fine_per_coarse)
        elif self.packed_bits:
            out.add("one-level packed (COUNT only)" if not self.accumulators else "one-level packed (one unsigned input)")
        else:
            out.add("one-level unpacked, %d accumulators" % len(self.accumulators))
        return out


def _nullable(seg, fq, column):
    return fq.null_handling and column >= 0 and seg.cols[column].nulls is not None


def key_cards(seg, fq):
    return [seg.cols[g].key_scale()[2] + (1 if _nullable(seg, fq, g) else 0) for g in fq.group_by]


def _int32_domain(col, kind):
    """An accumulator the 32-bit record format holds: MIN / MAX of any dictionary column fold dictIds; a SUM needs INT values, or a LONG
    dictionary whose range fits 31 bits (an offset dictionary: the 32-bit machinery applies to value - min, pg_segment_open in pg_engine.hip)."""
    if col.kind == F.RAW_INT or col.kind == F.DICT_INT or (kind != "sum" and col.is_dict):
        return True
    return col.kind == F.DICT_LONG and int(col.dict_values[-1]) - int(col.dict_values[0]) < 2 ** 31


LDS_TABLE_BYTES = 96 * 1024                       # pg_engine.hip size_group_launch  in_lds = table_bytes <= 96 * 1024 (group_private_kernel's LDS table)


def _lane_plan(seg, product, map_based, accumulators):
    """(partitionable, log2_fine_per_coarse) of one launch.  partitionable is None -- not foretold -- for a map-based key space whose
    table still fits group_private_kernel's LDS (10 001 .. 12 288 keys under COUNT alone): such a query may be answered by the LDS
    kernels before the partition decision is taken (run_group_by's batch deferral), depending on its filter."""
    k = plan(product, len(accumulators))[2]
    partitionable = (map_based and len(accumulators) <= MAX_PARTITION_AGGS and (1 << k) <= MAX_FINE_PER_COARSE and
                     all(_int32_domain(seg.cols[c], kind) for c, kind in accumulators))
    if partitionable and product * 8 * (1 + len(accumulators)) <= LDS_TABLE_BYTES:
        partitionable = None
    return partitionable, k


def describe(seg, fq):
    cols, info = seg.cols, GroupInfo()
    cards = key_cards(seg, fq)
    info.product = int(np.prod(cards))
    lanes = any(_nullable(seg, fq, c) for _, c in fq.aggs)
    first_appearance_keys = lanes or any(_nullable(seg, fq, g) for g in fq.group_by) or any(not cols[g].is_dict for g in fq.group_by)
    limit = fq.limit if fq.limit > 0 else DEFAULT_GROUPS_LIMIT
    info.first_appearance = first_appearance_keys and limit < info.product
    info.map_based = info.product > ARRAY_BASED_THRESHOLD or info.first_appearance
    kinds = {Q.SUM: "sum", Q.AVG: "sum", Q.MIN: "min", Q.MAX: "max"}
    info.accumulators = sorted({(c, kinds[f]) for f, c in fq.aggs if f != Q.COUNT and not (lanes and _nullable(seg, fq, c))})
    info.int32_inputs = all(_int32_domain(cols[c], kind) for c, kind in info.accumulators)
    info.shift, info.fine_partitions, info.log2_fine_per_coarse, info.scatter_partitions = plan(info.product, len(info.accumulators))
    info.klass = "lds" if info.product <= ARRAY_BASED_THRESHOLD else ("wide" if info.product > WIDE_KEYS else ("two-level" if info.log2_fine_per_coarse else "one-level"))
    info.partitionable = _lane_plan(seg, info.product, info.map_based, info.accumulators)[0]
    info.lane_plans = [(info.partitionable, info.log2_fine_per_coarse)]
    if lanes:       # a nullable column's lane: its own aggregations, every group of its own (no limit: the base lane decides which exist)
        for c in sorted({c for _, c in fq.aggs if _nullable(seg, fq, c)}):
            info.lane_plans.append(_lane_plan(seg, info.product, info.product > ARRAY_BASED_THRESHOLD, sorted({(c, kinds[f]) for f, cc in fq.aggs if cc == c and f != Q.COUNT})))
    info.packed_bits = 0
    scatter_shift = info.shift + info.log2_fine_per_coarse
    if not info.accumulators:
        info.packed_bits = 1
    elif len(info.accumulators) == 1:
        c, kind = info.accumulators[0]
        # an unsigned field: the dictId (MIN / MAX) or the value-plane field of an affine dictionary (SUM), which IS the dictId stream
        if cols[c].is_dict and (kind != "sum" or (_int32_domain(cols[c], kind) and _plane_bits(cols[c].dict_values)[1])) and cols[c].column.bits + scatter_shift <= 32:
            info.packed_bits = int(cols[c].column.bits)
    return info


def raw_keys(seg, fq):
    """The raw key of every doc as the result rows carry it: sum digit_c * prod(cardinalities before c); the NULL digit is the cardinality."""
    raw, mult = np.zeros(seg.n, dtype=np.int64), 1
    for g, card in zip(fq.group_by, key_cards(seg, fq)):
        digit = seg.digits[g]
        if _nullable(seg, fq, g):
            digit = np.where(seg.cols[g].nulls, card - 1, digit)
        raw += digit * mult
        mult *= card
    return raw


# ------------------------------------------------------------------------------------------------------------------------------------
# queries
# ------------------------------------------------------------------------------------------------------------------------------------
def _aggregations(rng, seg, shape):
    r = seg.roles
    signed = [r["irregular"], r["edges"], r["raw"]]
    int32 = signed + [r["affine"]]
    if shape in ("count", "lds") and (shape == "count" or rng.integers(0, 2)):
        return [(Q.COUNT, -1)]
    if shape == "unsigned1":                # the dictId of ANY dictionary column under MIN / MAX; the affine dictionary's plane field under SUM
        f = F._pick(rng, [Q.MIN, Q.MAX, Q.SUM, Q.AVG])
        c = r["affine"] if f in (Q.SUM, Q.AVG) else F._pick(rng, [r["affine"], r["irregular"], r["edges"], r["long"], r["benign"], r["ill"]])
        return [(f, c)] + ([(Q.COUNT, -1)] if rng.integers(0, 2) else [])
    if shape == "signed1":                  # a gathered dictionary value or a raw value: sign extension in pass B
        c = F._pick(rng, signed)
        return [(F._pick(rng, [Q.SUM, Q.AVG] if c != r["raw"] else [Q.SUM, Q.MIN, Q.MAX]), c)] + ([(Q.SUM, c)] if rng.integers(0, 2) else [])
    if shape == "min_max_sum":
        c = F._pick(rng, int32)
        return [(Q.MIN, c), (Q.MAX, c), (Q.SUM, c)] + ([(Q.AVG, c)] if rng.integers(0, 2) else [])
    if shape in ("two", "three"):
        want, aggs = 2 if shape == "two" else 3, []
        while len({(c, "s" if f in (Q.SUM, Q.AVG) else f) for f, c in aggs if f != Q.COUNT}) < want:
            aggs.append((F._pick(rng, [Q.SUM, Q.MIN, Q.MAX, Q.AVG]), F._pick(rng, int32)))
            aggs = aggs[-5:]
        return aggs
    if shape == "many":                     # four or five accumulators: beyond the record format
        c0, c1 = (int32[i] for i in rng.permutation(len(int32))[:2])
        return [(Q.SUM, c0), (Q.MIN, c0), (Q.MAX, c0), (Q.SUM, c1), (Q.MIN, c1)][: int(rng.integers(4, 6))]
    if shape == "wide_sum":                 # a LONG / DOUBLE sum: outside the 32-bit record format
        return [(F._pick(rng, [Q.SUM, Q.AVG]), F._pick(rng, [r["long"], r["benign"], r["ill"]]))] + [(F._pick(rng, F.FUNCTIONS[1:]), F._pick(rng, int32)) for _ in range(int(rng.integers(0, 3)))]
    everything = int32 + [r["long"], r["benign"], r["ill"]]
    return [(int(f), -1 if f == Q.COUNT else F._pick(rng, everything)) for f in rng.choice(F.FUNCTIONS, int(rng.integers(1, 6)))]


def _fixed_filter(seg, kind, rng):
    n = seg.n
    if kind == "nothing":
        return ("leaf", F.Leaf("match_none", Q.Pred(_abi.PG_PRED_MATCH_NONE)))
    lo, hi = ((n - 1) // TILE_DOCS * TILE_DOCS, n - 1) if kind == "last_tile" else (int(rng.integers(0, n)),) * 2
    return ("leaf", F.Leaf("doc_range", Q.Pred.doc_range(lo, hi), column=0, lo=lo, hi=hi))


def _make_query(rng, seg, shape, qi):
    null_handling = bool(rng.integers(0, 4) == 0) and shape != "lds"
    if shape == "lds":
        group_by = list(seg.small_keys)
    else:
        group_by = list(seg.keys)
    aggs = _aggregations(rng, seg, shape)
    if null_handling and rng.integers(0, 2):
        aggs = aggs + [(Q.COUNT, F._pick(rng, sorted(seg.roles.values())))]
    aggs = aggs[:5]
    tree, filter_kind = None, "none"
    style = int(rng.integers(0, 8))
    if (qi + seg.seed) % 4 == 1:            # every fixed kind in every segment, on a shape the partitioned path takes
        filter_kind = FIXED_FILTERS[(qi // 4 + seg.seed) % 3]
        tree = _fixed_filter(seg, filter_kind, rng)
    elif style >= 3:
        filter_kind = "tree"
        while True:
            made = []
            tree = F._make_tree(rng, seg, 2, True, made)
            if len(made) <= F.MAX_LEAVES:
                break
    fq = F.FuzzQuery(aggs, tree, group_by, null_handling, 0)
    fq.shape, fq.filter_kind = shape, filter_kind
    # num_groups_limit: 0, 5, 200, the groups present, one less
    how = int(rng.integers(0, 6))
    if how >= 2 and shape != "lds":
        present = len(F.expected(seg, fq).groups)
        limit = {2: 5, 3: 200, 4: present, 5: present - 1}[how]
        if limit > 0:
            fq = F.FuzzQuery(aggs, tree, group_by, null_handling, limit)
            fq.shape, fq.filter_kind = shape, filter_kind
        fq.limit_kind = {2: "5", 3: "200", 4: "present", 5: "present-1"}[how] if limit > 0 else "0"
    else:
        fq.limit_kind = "0"
    fq.info = describe(seg, fq)
    return fq


def make_queries(seg):
    rng = np.random.default_rng(66_000 + SEED_BASE + seg.seed)
    return [_make_query(rng, seg, shape, qi) for qi, shape in enumerate(QUERY_SHAPES)]


def static_decline(seg, fq):
    """The documented decline (a pattern of F.DECLINE_ALLOW_LIST) a query matches by its own shape, or None: the conditions the
    generator avoids by construction, stated once more as a check."""
    cols = seg.cols
    for g in fq.group_by:
        if fq.null_handling and not cols[g].is_dict and cols[g].nulls is not None:
            return "GROUP BY over nullable raw column"
        if not cols[g].is_dict and cols[g].key_scale()[0] != "offset":
            return "group-by with raw keys beyond an int"
    if int(np.prod(key_cards(seg, fq))) >= 2 ** 31:
        return "group-by with raw keys beyond an int"
    for f, c in fq.aggs:
        if c < 0 or f == Q.COUNT:
            continue
        if f in (Q.SUM, Q.AVG) and cols[c].kind in (F.DICT_LONG, F.RAW_LONG) and (not cols[c].sum_safe or seg.n * float(np.abs(cols[c].values.astype(np.float64)).max()) >= 9.2e18):
            return "group-by SUM of LONG column could overflow int64"
        if f == Q.MAX and cols[c].is_dict and cols[c].is_fp and cols[c].has("nan"):
            return "group-by MAX of dictionary column whose dictionary holds NaN"
        if cols[c].is_wide_raw:
            return "group-by aggregation of a raw 8-byte column"
    if len(fq.leaves()) > F.MAX_LEAVES:
        return "more than 8 filter leaves"
    if len({(c, f if f in (Q.MIN, Q.MAX) else Q.SUM) for f, c in fq.aggs if f != Q.COUNT}) > 8:
        return "more than 8 distinct group-by aggregations"
    referenced = set(fq.group_by) | {c for _, c in fq.aggs if c >= 0} | {x.column for x in fq.leaves() if x.kind not in ("match_all", "match_none", "doc_range")}
    if len(referenced) > 16:
        return "query references more than 16 columns"
    return None
