"""Randomised segments and queries over every column encoding and filter-leaf kind the engine has, and an EXACT MODEL of what each query
returns -- shared by tests/test_fuzz_cases_cpu.py (oracle vs. model) and tests/test_gpu_fuzz_typed.py (device vs. oracle and model).
Nothing here needs a GPU or the oracle.  Deterministic in (seed); PINOT_FUZZ_SEED_BASE shifts every seed, as in tests/test_gpu_fuzz.py.

Segments: `num_docs` around the 64-doc step, the 2048-doc tile and beyond one tile per wave (SIZES); 6-10 columns out of dictionary INT
(natural and forced widths, affine and irregular dictionaries), dictionary INT over the type's edges, a sorted dictionary column, a
dictionary column with an inverted index, dictionary LONG (offset-able and wide), dictionary FLOAT / DOUBLE, raw INT / LONG / FLOAT /
DOUBLE; null value vectors (sparse / dense / one run) on some.  Value pools are small -- groups and set members repeat -- and hold the edges
by default: INT -2^31, -1, 0, 1, 2^31-1; LONG -2^63, -2^32, -1, 0, 1, 2^32, 2^63-1; FLOAT / DOUBLE NaN, +-inf, +-0.0, the smallest
subnormals, the largest finite value, 0.1, 16777217.  Sum-safe LONG columns keep |v| <= 2^40.  Floating-point columns come in three
flavours (Col.pool): "benign" (finite, zeros included), "special" (NaN / +-inf present: a sum over them is NaN or an infinity by IEEE
rules in ANY order -- the largest finite value only goes with columns that hold no -inf, so that no order of additions can meet
+inf + -inf through an overflow), "ill" (finite, every magnitude with both signs so that sum|x| >> |sum x|: magnitudes 1e-30 .. 1e30, or
all within a factor two of 1e15, where losing or doubling one value is far outside the bound the tests hold a sum to).

Queries: leaves dict_range, dict_set, doc_range, the inverted forms, is_null, match_all / match_none, raw_range (raw INT / LONG; bounds
from the pool, lo > hi, the full range), raw_range_f64 (raw FLOAT / DOUBLE; +-0.0, +-inf, lo > hi), raw_set / raw_set_f64 (1 ..
PG_RAW_SET_MAX_VALUES values, present and absent, duplicates, exclusive); trees of depth <= 2 with at most 8 leaves, sometimes one Pred
object behind two leaves; 1-5 aggregations; no group-by or 1-2 keys of any column kind; null_handling; num_groups_limit.

What the generator does NOT produce, and why:
  * FP IN lists with a zero or a NaN: declined by design ("IN list on raw column %s holds a zero or a NaN", pg_engine.hip lower_raw_set);
    tests/test_gpu_raw_in.py::test_declines keeps them.
  * `S.Column.dict_encoded_typed` builds dictionaries with np.unique, which merges -0.0 and 0.0; the reference's dictionaries
    (Double.compare order) keep both.  The fuzz therefore does NOT cover two-zero dictionaries: a dictionary column here stores one zero.
  * GROUP BY with MIN / MAX over a FLOAT / DOUBLE column that holds NaN under enableNullHandling: the reference is order dependent there
    (`result == null || value < result`, MinAggregationFunction.java:168-178: a NaN that is the group's first non-null value sticks, a
    later one is ignored).  group_min / group_max below state the rule without null handling; with it the generator keeps NaN columns out.
  * hashed holders (raw keys beyond an int): two keys over small pools never get there; tests/hash_holder_cases.py does.
  * the plan-time fallbacks the engine documents (pg_engine.hip, `fail(PG_ERR_UNSUPPORTED, ...)`), avoided by construction:
      - "group-by aggregation of a raw 8-byte column under a raw 8-byte range predicate (plan-time fallback)": a group-by that aggregates a
        raw LONG / FLOAT / DOUBLE column gets no raw_range leaf on a raw LONG / FLOAT / DOUBLE column;
      - "group-by with raw keys beyond an int under null handling" / "... under a raw 8-byte range predicate": no hashed holders at all;
      - "GROUP BY over nullable raw column %s keeps the CPU plan": under null handling a raw key column has no null vector (the oracle
        declines rank-keyed columns under null handling too: those are not keys then);
      - "group-by SUM of LONG column %s could overflow int64": group-by SUM / AVG only over sum-safe LONG columns;
      - "more than 8 filter leaves", "filter tree has %d nodes", "filter tree deeper than %d", "query references more than 16 columns",
        "more than 4 aggregated columns", "more than 8 distinct group-by aggregations": the trees, column counts and aggregation lists
        stay below every cap.
  * NOT avoided, so that the decline itself stays under test: "group-by MAX of dictionary column %s whose dictionary holds NaN" -- the
    group kernels fold dictIds, the NaN entry is the largest, and the reference's `value > holder` skips NaN.
    DECLINE_ALLOW_LIST below is what a device decline may still say; the GPU test caps them at 10 % of all generated queries."""
import math
import os

import numpy as np

from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S

SEED_BASE = int(os.environ.get("PINOT_FUZZ_SEED_BASE", "0"))
SEEDS = list(range(24))
QUERIES_PER_SEGMENT = 12
SIZES = [1, 63, 64, 65, 2047, 2048, 2049, 4097, 20_011, 70_001, 140_000]
CAP = _abi.PG_RAW_SET_MAX_VALUES
MAX_LEAVES = 8
MAX_AGG_COLUMNS = 4              # kMaxAggCols: distinct aggregated columns of an aggregation-only query
MAX_GROUPS = 60_000              # product of the key cardinalities the generator stays below
ARRAY_BASED_THRESHOLD = 10_000   # DictionaryBasedGroupKeyGenerator.java:150-184: above it the holder is map based and numGroupsLimit binds
DEFAULT_GROUPS_LIMIT = 100_000   # InstancePlanMakerImplV2.DEFAULT_NUM_GROUPS_LIMIT

# the documented fallbacks a generated query may still run into (regular expressions over pg_last_error)
DECLINE_ALLOW_LIST = [
    r"group-by aggregation of a raw 8-byte column under a raw 8-byte range predicate",
    r"group-by with raw keys beyond an int",
    r"GROUP BY over nullable raw column",
    r"group-by SUM of LONG column \S+ could overflow int64",
    r"group-by MAX of dictionary column \S+ whose dictionary holds NaN",
    r"more than \d+ filter leaves", r"filter tree has \d+ nodes", r"filter tree deeper than \d+",
    r"query references more than \d+ columns", r"more than \d+ aggregated columns", r"more than \d+ distinct group-by aggregations",
    r"query needs \d+ bytes of LDS per wavefront", r"group-by table of \d+ slots",
    r"IN list on raw column \S+: no table of \d+ bytes places its \d+ values",
]

DICT_INT, DICT_LONG, DICT_FLOAT, DICT_DOUBLE = "dict_int", "dict_long", "dict_float", "dict_double"
RAW_INT, RAW_LONG, RAW_FLOAT, RAW_DOUBLE = "raw_int", "raw_long", "raw_float", "raw_double"
KINDS = [DICT_INT, DICT_LONG, DICT_FLOAT, DICT_DOUBLE, RAW_INT, RAW_LONG, RAW_FLOAT, RAW_DOUBLE]
DTYPES = {DICT_INT: np.int32, DICT_LONG: np.int64, DICT_FLOAT: np.float32, DICT_DOUBLE: np.float64,
          RAW_INT: np.int32, RAW_LONG: np.int64, RAW_FLOAT: np.float32, RAW_DOUBLE: np.float64}
INT_EDGES = [-2 ** 31, -1, 0, 1, 2 ** 31 - 1]
LONG_EDGES = [-2 ** 63, -2 ** 32, -1, 0, 1, 2 ** 32, 2 ** 63 - 1]
LONG_SAFE_EDGES = [-2 ** 40, -2 ** 32, -1, 0, 1, 2 ** 32, 2 ** 40]
FUNCTIONS = [Q.COUNT, Q.SUM, Q.MIN, Q.MAX, Q.AVG]
U = 2.0 ** -53                   # unit roundoff of a double


class Col:
    """One column as the model sees it: the stored VALUES (`values`, the numpy array of the stored type), the dictIds and dictionary of
    a dictionary column, the null mask or None, and what the generator may do with it."""

    def __init__(self, name, kind, values, column, ids=None, dict_values=None, pool=None, sum_safe=True, is_sorted=False):
        self.name, self.kind, self.values, self.column = name, kind, values, column
        self.ids, self.dict_values = ids, dict_values
        self.pool, self.sum_safe, self.is_sorted = pool, sum_safe, is_sorted
        self.nulls = None

    is_dict = property(lambda self: self.ids is not None)
    is_fp = property(lambda self: self.kind in (DICT_FLOAT, DICT_DOUBLE, RAW_FLOAT, RAW_DOUBLE))
    is_wide_raw = property(lambda self: self.kind in (RAW_LONG, RAW_FLOAT, RAW_DOUBLE))        # "raw 8-byte" in the engine's messages: not INT
    inverted = property(lambda self: self.column.inverted is not None)
    cardinality = property(lambda self: self.column.cardinality)

    def doubles(self):
        """getDoubleValuesSV: FLOAT widens exactly, LONG rounds to nearest."""
        return self.values.astype(np.float64)

    def has(self, what):
        d = self.doubles()
        return bool({"nan": np.isnan(d).any(), "inf": np.isinf(d).any(), "zero": (d == 0.0).any()}[what]) if len(d) else False

    def key_scale(self):
        """How a GROUP BY digit of this column maps to a value (include/pinot_gpu.h, pg_group_key_info): ("dict", dictionary) the dictId;
        ("offset", base) value - min of a raw INT / LONG column whose range fits an int; ("rank", identities ascending) the rank among the
        column's distinct values otherwise (FLOAT / DOUBLE, wider ranges).  Also the digit count."""
        if self.is_dict:
            return "dict", self.dict_values, int(self.cardinality)
        if not self.is_fp:
            lo, hi = int(self.values.min()), int(self.values.max())
            if hi - lo < 0x7FFFFFFE:
                return "offset", lo, hi - lo + 1
        ident = np.unique(key_identity(self.values))
        order = np.where(ident < 0, ~ident, ident | np.int64(-(2 ** 63))).view(np.uint64) if self.is_fp else ident
        ident = ident[np.argsort(order, kind="stable")]
        return "rank", ident, len(ident)


def key_identity(values):
    """What makes two values the SAME group key in the reference's maps, as int64: the long; Double.doubleToLongBits of the widened
    double -- one NaN, -0.0 and 0.0 apart (NoDictionarySingleColumnGroupKeyGenerator.java:100-135)."""
    values = np.asarray(values)
    if np.issubdtype(values.dtype, np.floating):
        d = values.astype(np.float64)
        bits = d.view(np.int64).copy()
        bits[np.isnan(d)] = np.int64(0x7FF8000000000000)
        return bits
    return values.astype(np.int64)


class Segment:
    def __init__(self, seed, n, cols):
        self.seed, self.n, self.cols = seed, n, cols
        self.data = S.SegmentData("fuzzt%d" % seed, n, [c.column for c in cols])


# ------------------------------------------------------------------------------------------------------------------------------------
# segments
# ------------------------------------------------------------------------------------------------------------------------------------
def _fp_pool(rng, dtype, flavour):
    fi = np.finfo(dtype)
    tiny = np.array([fi.smallest_subnormal, -fi.smallest_subnormal], dtype=dtype)
    with np.errstate(over="ignore"):
        if flavour == "ill":
            k = int(rng.integers(3, 9))
            mags = (10.0 ** rng.uniform(-30, 30, k)) if rng.integers(0, 2) else rng.uniform(1e15, 2e15, k)
            mags = mags.astype(dtype)
            return np.concatenate([mags, -mags]).astype(dtype)
        body = np.concatenate([rng.uniform(-1e5, 1e6, int(rng.integers(3, 20))), [0.1, 16777217.0, 0.0, -0.0]]).astype(dtype)
        body = np.concatenate([body, tiny])
        if flavour == "benign":
            return body
        specials = [[np.nan], [np.inf], [-np.inf], [np.nan, np.inf], [np.nan, -np.inf], [np.inf, -np.inf], [np.nan, np.inf, -np.inf]][int(rng.integers(0, 7))]
        if -np.inf not in specials and rng.integers(0, 2):
            specials = specials + [float(fi.max)]
        return np.concatenate([body, np.array(specials, dtype=dtype)])


def _forced_width_dict_int(rng, name, n, with_inverted):
    """A `card`-entry INT dictionary packed at `bits` >= the natural width (tests/test_gpu_fuzz.py's columns)."""
    card = int(rng.choice([2, 3, 7, 64, 1000, 5000]))
    natural = max(1, int(np.ceil(np.log2(card))))
    bits = int(rng.integers(natural, 32)) if rng.integers(0, 2) else natural
    if rng.integers(0, 2):
        values = (np.arange(card, dtype=np.int64) * int(rng.integers(1, 9)) + int(rng.integers(-1000, 1000))).astype(np.int32)
    else:
        values = np.sort(rng.choice(np.arange(-2 ** 20, 2 ** 20, dtype=np.int64), card, replace=False)).astype(np.int32)
    ids = rng.integers(0, card, n).astype(np.int32)
    col = S.Column.from_dict_ids(name, values, ids, with_inverted=with_inverted)
    if bits > col.bits:
        host = S.load_host_library()
        col.bits = bits
        col.fwd = np.zeros(int(host.ph_fixedbit_size(n, bits)), dtype=np.uint8)
        host.ph_fixedbit_pack(S._i32p(ids), n, bits, S._u8p(col.fwd), 2)
    return Col(name, DICT_INT, values[ids], col, ids=ids, dict_values=values)


def _typed_dict(name, kind, drawn, with_inverted=False, **kw):
    """np.unique's dictionary (ascending, one NaN last, ONE zero) and the values the column then stores."""
    dict_values, ids = np.unique(drawn, return_inverse=True)
    dict_values = np.ascontiguousarray(dict_values, dtype=drawn.dtype)
    stored = dict_values[ids]
    col = S.Column.dict_encoded_typed(name, stored, with_inverted=with_inverted)
    assert col.cardinality == len(dict_values)
    return Col(name, kind, stored, col, ids=np.ascontiguousarray(ids, dtype=np.int32), dict_values=dict_values, **kw)


def _draw(rng, pool, n):
    pool = np.asarray(pool)
    return pool[rng.integers(0, len(pool), n)]


def _make_column(rng, recipe, name, n):
    if recipe == "dict_int_forced":
        return _forced_width_dict_int(rng, name, n, with_inverted=False)
    if recipe == "dict_int_inverted":
        return _forced_width_dict_int(rng, name, n, with_inverted=True) if rng.integers(0, 2) else \
            _typed_dict(name, DICT_INT, _draw(rng, np.arange(12, dtype=np.int32) * 5 - 7, n), with_inverted=True)
    if recipe == "dict_int_edges":
        pool = np.array(INT_EDGES + [int(x) for x in rng.integers(-2 ** 31, 2 ** 31, int(rng.integers(1, 25)))], dtype=np.int32)
        return _typed_dict(name, DICT_INT, _draw(rng, pool, n))
    if recipe == "dict_int_sorted":
        c = _typed_dict(name, DICT_INT, np.sort(rng.integers(0, int(rng.choice([2, 9, 50])), n)).astype(np.int32) * 3 - 11)
        c.is_sorted = True
        return c
    if recipe in (DICT_LONG, RAW_LONG):
        flavour = int(rng.integers(0, 3))
        if flavour == 0:        # offset-able: a narrow band far from zero (an offset dictionary / an int-range key image)
            base = int(rng.choice([-1, 1])) * (2 ** 40 - 5000)
            pool, safe = base + rng.integers(0, 41 if recipe == RAW_LONG else 1000, int(rng.integers(2, 30))), True
        elif flavour == 1:
            pool, safe = LONG_SAFE_EDGES + [int(x) for x in rng.integers(-2 ** 40, 2 ** 40, int(rng.integers(1, 20)))], True
        else:
            pool, safe = LONG_EDGES + [int(x) for x in rng.integers(-2 ** 63, 2 ** 63 - 1, int(rng.integers(1, 20)), dtype=np.int64)], False
        drawn = _draw(rng, np.array(pool, dtype=np.int64), n)
        if recipe == DICT_LONG:
            return _typed_dict(name, DICT_LONG, drawn, sum_safe=safe)
        return Col(name, RAW_LONG, drawn, S.Column.raw_typed(name, drawn), sum_safe=safe)
    if recipe == RAW_INT:
        pool = (np.arange(41) - 20) * int(rng.integers(1, 4)) if rng.integers(0, 2) else np.array(INT_EDGES + [int(x) for x in rng.integers(-2 ** 31, 2 ** 31, int(rng.integers(1, 25)))])
        drawn = _draw(rng, pool.astype(np.int32), n)
        return Col(name, RAW_INT, drawn, S.Column.raw(name, drawn))
    dtype = DTYPES[recipe]
    flavour = ["benign", "special", "special", "ill", "ill"][int(rng.integers(0, 5))]
    drawn = _draw(rng, _fp_pool(rng, dtype, flavour), n).astype(dtype)
    if recipe in (DICT_FLOAT, DICT_DOUBLE):
        return _typed_dict(name, recipe, drawn, with_inverted=bool(rng.integers(0, 4) == 0), pool=flavour)
    return Col(name, recipe, drawn, S.Column.raw_typed(name, drawn), pool=flavour)


RECIPES = ["dict_int_forced", "dict_int_inverted", "dict_int_edges", "dict_int_sorted", DICT_LONG, DICT_FLOAT, DICT_DOUBLE, RAW_INT, RAW_LONG, RAW_FLOAT, RAW_DOUBLE,
           RAW_FLOAT, RAW_DOUBLE, DICT_DOUBLE, RAW_LONG, RAW_INT, DICT_LONG, DICT_FLOAT]


def make_segment(seed):
    rng = np.random.default_rng(77_000 + SEED_BASE + seed)
    n = SIZES[seed % len(SIZES)] if seed < 2 * len(SIZES) else int(rng.choice(SIZES))
    recipes = ["dict_int_inverted"] + [RECIPES[i] for i in rng.permutation(len(RECIPES))[: int(rng.integers(5, 10))]]
    cols = []
    for i, recipe in enumerate(recipes):
        c = _make_column(rng, recipe, "c%d" % i, n)
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
        cols.append(c)
    return Segment(seed, n, cols)


# ------------------------------------------------------------------------------------------------------------------------------------
# queries
# ------------------------------------------------------------------------------------------------------------------------------------
class Leaf:
    """One predicate: `kind` (a name of LEAF_KINDS), the column, what it matches (`args`), and the Pred object handed to the engine."""

    def __init__(self, kind, pred, column=-1, exclusive=False, **args):
        self.kind, self.pred, self.column, self.exclusive, self.args = kind, pred, column, exclusive, args


LEAF_KINDS = ["dict_range", "dict_set", "doc_range", "inverted_range", "inverted_set", "is_null", "match_all", "match_none",
              "raw_range", "raw_range_f64", "raw_set", "raw_set_f64"]


class FuzzQuery:
    def __init__(self, aggs, tree, group_by, null_handling, limit):
        self.aggs, self.tree, self.group_by, self.null_handling, self.limit = aggs, tree, group_by, null_handling, limit
        self.spec = Q.QuerySpec(aggs, filter=_to_node(tree) if tree is not None else None, group_by=group_by, null_handling=null_handling, num_groups_limit=limit)

    def leaves(self):
        out = []

        def walk(t):
            if t[0] == "leaf":
                out.append(t[1])
            else:
                for ch in t[1]:
                    walk(ch)
        if self.tree is not None:
            walk(self.tree)
        return out


def _to_node(t):
    if t[0] == "leaf":
        return Q.leaf(t[1].pred)
    kids = [_to_node(ch) for ch in t[1]]
    return Q.not_(kids[0]) if t[0] == "not" else (Q.and_(*kids) if t[0] == "and" else Q.or_(*kids))


def _pick(rng, items):
    return items[int(rng.integers(0, len(items)))]


def _set_values(rng, col, fp):
    """An IN list: 1 .. CAP distinct values, present (from the column) and absent, sometimes with a duplicate; FP lists without zero / NaN."""
    size = int(rng.choice([1, 1, 2, 5, 17, 100, CAP]))
    present = np.unique(col.values.astype(np.float64) if fp else col.values.astype(np.int64))
    if fp:
        present = present[np.isfinite(present) & (present != 0.0)] if rng.integers(0, 4) else present[~np.isnan(present) & (present != 0.0)]
    present = [v.item() for v in present[rng.permutation(len(present))[: max(1, min(size, len(present)) - int(rng.integers(0, 2)))]]]
    values = list(present)
    lo, hi = (-2 ** 31, 2 ** 31) if col.kind == RAW_INT else (-2 ** 62, 2 ** 62)
    while len(set(values)) < size:
        if fp:
            v = float(rng.choice([0.1, 1e-320, 12345.678, -7.25e-20, 3e300])) if rng.integers(0, 3) == 0 else float(rng.normal(0, 1e6))
            if v == 0.0:
                continue
        else:
            v = int(rng.integers(lo, hi))
        values.append(v)
    values = list(dict.fromkeys(values))[:size]
    if len(values) < CAP and rng.integers(0, 3) == 0:
        values.append(values[0])              # a duplicate: the engine de-duplicates
    return [values[i] for i in rng.permutation(len(values))]


def _make_leaf(rng, seg, allow_wide_raw_range, kind=None, only=None):
    """`kind` / `only`: the leaf kind and the column kinds to take (the lean shapes); otherwise any kind the segment has a column for."""
    n = seg.n
    excl = bool(rng.integers(0, 4) == 0)
    kind = kind or _pick(rng, ["dict_range", "dict_range", "dict_set", "dict_set", "doc_range", "inverted_range", "inverted_set", "is_null", "match_all", "match_none",
                               "raw_range", "raw_range", "raw_range_f64", "raw_range_f64", "raw_set", "raw_set", "raw_set_f64", "raw_set_f64"])
    by = {
        "dict_range": [i for i, c in enumerate(seg.cols) if c.is_dict], "dict_set": [i for i, c in enumerate(seg.cols) if c.is_dict],
        "inverted_range": [i for i, c in enumerate(seg.cols) if c.is_dict and c.inverted], "inverted_set": [i for i, c in enumerate(seg.cols) if c.is_dict and c.inverted],
        "raw_range": [i for i, c in enumerate(seg.cols) if c.kind == RAW_INT or (c.kind == RAW_LONG and allow_wide_raw_range)],
        "raw_range_f64": [i for i, c in enumerate(seg.cols) if c.kind in (RAW_FLOAT, RAW_DOUBLE) and allow_wide_raw_range],
        "raw_set": [i for i, c in enumerate(seg.cols) if c.kind in (RAW_INT, RAW_LONG)], "raw_set_f64": [i for i, c in enumerate(seg.cols) if c.kind in (RAW_FLOAT, RAW_DOUBLE)],
    }
    if only is not None:
        by = {k: [i for i in v if seg.cols[i].kind in only] for k, v in by.items()}
    if kind in by and not by[kind]:
        kind = "doc_range"
    if kind in ("match_all", "match_none"):
        return Leaf(kind, Q.Pred(_abi.PG_PRED_MATCH_ALL if kind == "match_all" else _abi.PG_PRED_MATCH_NONE, exclusive=excl), exclusive=excl)
    if kind == "doc_range":
        lo = int(rng.integers(-5, n + 5))
        hi = lo + int(rng.integers(0, n + 1))
        return Leaf(kind, Q.Pred.doc_range(lo, hi, exclusive=excl), column=0, exclusive=excl, lo=lo, hi=hi)      # (Pred.doc_range names column 0)
    if kind == "is_null":
        ci = int(rng.integers(0, len(seg.cols)))
        return Leaf(kind, Q.Pred.is_null(ci, exclusive=excl), column=ci, exclusive=excl)
    ci = _pick(rng, by[kind])
    col = seg.cols[ci]
    if kind in ("dict_range", "inverted_range"):
        card = col.cardinality
        lo = int(rng.integers(0, card))
        hi = int(rng.integers(lo, card + 1))
        if hi == lo:
            hi = min(card, lo + 1)
        if kind == "inverted_range":
            hi = min(hi, lo + 3)
        return Leaf(kind, Q.Pred.dict_range(ci, lo, hi, exclusive=excl, inverted=kind == "inverted_range"), column=ci, exclusive=excl, lo=lo, hi=hi)
    if kind in ("dict_set", "inverted_set"):
        card = col.cardinality
        ids = sorted(set(int(x) for x in rng.integers(0, card, int(rng.integers(1, 6)))))
        return Leaf(kind, Q.Pred.dict_set(ci, ids, card, exclusive=excl, inverted=kind == "inverted_set"), column=ci, exclusive=excl, ids=ids)
    if kind == "raw_range":
        info = np.iinfo(col.values.dtype)
        style = int(rng.integers(0, 6))
        if style == 0:
            lo, hi = int(info.min), int(info.max)
        else:
            a, b = (int(_pick(rng, col.values)) + int(rng.integers(-1, 2)) for _ in range(2))
            a, b = (min(max(x, int(info.min)), int(info.max)) for x in (a, b))
            lo, hi = (max(a, b), min(a, b)) if style == 1 else (min(a, b), max(a, b))        # style 1: lo > hi (or a point)
        return Leaf(kind, Q.Pred.raw_range(ci, lo, hi, exclusive=excl), column=ci, exclusive=excl, lo=lo, hi=hi)
    if kind == "raw_range_f64":
        finite = col.doubles()[np.isfinite(col.doubles())]
        cands = [0.0, -0.0, np.inf, -np.inf] + ([float(_pick(rng, finite)) for _ in range(4)] if len(finite) else [1.0])
        a, b = float(_pick(rng, cands)), float(_pick(rng, cands))
        lo, hi = (max(a, b), min(a, b)) if rng.integers(0, 6) == 0 else (min(a, b), max(a, b))
        return Leaf(kind, Q.Pred.raw_range_f64(ci, lo, hi, exclusive=excl), column=ci, exclusive=excl, lo=lo, hi=hi)
    fp = kind == "raw_set_f64"
    values = _set_values(rng, col, fp)
    pred = Q.Pred.raw_set_f64(ci, values, exclusive=excl) if fp else Q.Pred.raw_set(ci, values, exclusive=excl)
    return Leaf(kind, pred, column=ci, exclusive=excl, values=values)


def _make_tree(rng, seg, depth, allow_wide_raw_range, made):
    if depth == 0 or rng.integers(0, 3) == 0:
        if made and rng.integers(0, 8) == 0:
            leaf = _pick(rng, made)                 # ONE Pred object behind two leaves
        else:
            leaf = _make_leaf(rng, seg, allow_wide_raw_range)
        made.append(leaf)
        return ("leaf", leaf)
    op = int(rng.integers(0, 3))
    if op == 2:
        return ("not", [_make_tree(rng, seg, depth - 1, allow_wide_raw_range, made)])
    return ("and" if op == 0 else "or", [_make_tree(rng, seg, depth - 1, allow_wide_raw_range, made) for _ in range(int(rng.integers(2, 4)))])


def _make_query(rng, seg):
    cols = seg.cols
    null_handling = bool(rng.integers(0, 3) == 0)
    group_by = []
    if seg.n > 0 and rng.integers(0, 5) < 2:
        def key_ok(c):
            scale = c.key_scale()
            if null_handling and not c.is_dict and (c.nulls is not None or scale[0] == "rank"):
                return False
            return scale[2] + 1 <= MAX_GROUPS
        eligible = [i for i, c in enumerate(cols) if key_ok(c)]
        if eligible:
            group_by = [int(x) for x in rng.choice(eligible, min(len(eligible), int(rng.integers(1, 3))), replace=False)]
            if np.prod([cols[g].key_scale()[2] + 1 for g in group_by]) > MAX_GROUPS:
                group_by = group_by[:1]
    aggs, agg_cols = [], []
    for f in rng.choice(FUNCTIONS, int(rng.integers(1, 6))):
        f = int(f)
        if f == Q.COUNT:
            aggs.append((f, int(rng.integers(0, len(cols))) if null_handling and rng.integers(0, 2) else -1))
            continue

        def agg_ok(i):
            c = cols[i]
            if not group_by:
                return i in agg_cols or len(agg_cols) < MAX_AGG_COLUMNS
            if f in (Q.SUM, Q.AVG) and c.kind in (DICT_LONG, RAW_LONG) and not c.sum_safe:
                return False
            if f in (Q.MIN, Q.MAX) and null_handling and c.is_fp and c.has("nan"):
                return False
            return True
        eligible = [i for i in range(len(cols)) if agg_ok(i)]
        if not eligible:
            continue
        ci = _pick(rng, eligible)
        if ci not in agg_cols:
            agg_cols.append(ci)
        aggs.append((f, ci))
    if group_by and not null_handling and rng.integers(0, 2):
        # what this fuzz exists for: a group's MIN / MAX over a column that holds NaN (and, with luck, a group of nothing else)
        with_nan = [i for i, c in enumerate(cols) if c.is_fp and c.has("nan")]
        if with_nan:
            ci = _pick(rng, with_nan)
            # (MAX over a dictionary that holds NaN is the engine's documented decline: the general draw above meets it often enough)
            aggs = aggs[:3] + [(Q.MIN, ci), (Q.MAX, ci)][: 1 if cols[ci].is_dict else 1 + int(rng.integers(0, 2))]
    if not aggs:
        aggs = [(Q.COUNT, -1)]
    allow_wide_raw_range = not (group_by and any(c >= 0 and cols[c].is_wide_raw for _, c in aggs))
    tree = None
    if rng.integers(0, 6):
        while True:
            made = []
            tree = _make_tree(rng, seg, 2, allow_wide_raw_range, made)
            if len(made) <= MAX_LEAVES:
                break
    limit = int(rng.choice([0, 0, 5, 200])) if group_by else 0
    return FuzzQuery(aggs, tree, group_by, null_handling, limit)


def _make_lean_query(rng, seg):
    """The shapes the specialised scan kernels exist for (choose_scan_kernel, pg_engine.hip): no group-by, no null handling, one leaf or
    none, at most one aggregated column -- a dictionary leaf before a dictionary INT column, a raw INT range or a raw IN list before a raw
    INT column, a small tree of dictionary leaves under COUNT(*) alone."""
    cols = seg.cols
    shape = _pick(rng, ["dict", "dict", "raw_range", "raw_range", "raw_set", "count"])
    if shape == "count":
        kids = [("leaf", _make_leaf(rng, seg, True, kind=_pick(rng, ["dict_range", "dict_set"]), only=(DICT_INT,))) for _ in range(int(rng.integers(1, 4)))]
        tree = kids[0] if len(kids) == 1 else (_pick(rng, ["and", "or"]), kids)
        return FuzzQuery([(Q.COUNT, -1)], tree, [], False, 0)
    want = DICT_INT if shape == "dict" else RAW_INT
    eligible = [i for i, c in enumerate(cols) if c.kind == want]
    if not eligible:
        return _make_query(rng, seg)
    ci = _pick(rng, eligible)
    aggs = [(int(f), -1 if f == Q.COUNT else ci) for f in rng.choice(FUNCTIONS, int(rng.integers(1, 4)))]
    tree = None
    if shape != "dict" or rng.integers(0, 4):
        kind = {"dict": _pick(rng, ["dict_range", "dict_range", "dict_set"]), "raw_range": "raw_range", "raw_set": "raw_set"}[shape]
        tree = ("leaf", _make_leaf(rng, seg, True, kind=kind, only=(DICT_INT,) if shape == "dict" else ((RAW_INT,) if shape == "raw_range" else (RAW_INT, RAW_LONG))))
    return FuzzQuery(aggs, tree, [], False, 0)


def make_queries(seg):
    rng = np.random.default_rng(91_000 + SEED_BASE + seg.seed)
    return [_make_lean_query(rng, seg) if rng.integers(0, 3) == 0 else _make_query(rng, seg) for _ in range(QUERIES_PER_SEGMENT)]


# ------------------------------------------------------------------------------------------------------------------------------------
# the exact model
# ------------------------------------------------------------------------------------------------------------------------------------
def leaf_matches(seg, leaf):
    """PredicateEvaluator.applySV over the column's values (exclusive = the NOT_EQ / NOT_IN / negated evaluator): primitive compares -- a
    NaN is in no range, -0.0 == 0.0 (RangePredicateEvaluatorFactory.java:331-560); set membership by value
    (InPredicateEvaluatorFactory.java:215-300; the lists hold no zero and no NaN, where Float / Double hash sets compare bits)."""
    n = seg.n
    k, a = leaf.kind, leaf.args
    if k == "match_all":
        m = np.ones(n, bool)
    elif k == "match_none":
        m = np.zeros(n, bool)
    elif k == "doc_range":
        d = np.arange(n)
        m = (d >= a["lo"]) & (d <= a["hi"])
    elif k == "is_null":
        nulls = seg.cols[leaf.column].nulls
        m = nulls.copy() if nulls is not None else np.zeros(n, bool)
    else:
        col = seg.cols[leaf.column]
        if k in ("dict_range", "inverted_range"):
            m = (col.ids >= a["lo"]) & (col.ids < a["hi"])
        elif k in ("dict_set", "inverted_set"):
            m = np.isin(col.ids, a["ids"])
        elif k == "raw_range":
            v = col.values.astype(object) if col.kind == RAW_LONG else col.values.astype(np.int64)
            m = np.asarray((v >= a["lo"]) & (v <= a["hi"]), dtype=bool)
        elif k == "raw_range_f64":
            with np.errstate(invalid="ignore"):
                m = (col.doubles() >= a["lo"]) & (col.doubles() <= a["hi"])
        elif k == "raw_set":
            m = np.isin(col.values.astype(np.int64), np.array(a["values"], dtype=np.int64))
        else:
            m = np.isin(col.doubles(), np.array(a["values"], dtype=np.float64))
    return ~m if leaf.exclusive else m


def filter_mask(seg, fq):
    """The filter's docs.  Without null handling: plain set algebra.  With it (tests/null_cases.py, BaseFilterOperator.java:85-113): a
    column leaf has trues = matches AND NOT nulls and nulls = the column's null docs; IS_NULL / MATCH_ALL / MATCH_NONE have no nulls;
    AND / OR combine trues and (trues OR nulls); NOT returns the child's falses."""
    n = seg.n
    if fq.tree is None:
        return np.ones(n, bool)

    def tnf(t):
        if t[0] == "leaf":
            leaf = t[1]
            m = leaf_matches(seg, leaf)
            nulls = None
            if fq.null_handling and leaf.kind not in ("is_null", "match_all", "match_none"):
                nulls = seg.cols[leaf.column].nulls
            if nulls is None:
                return m, np.zeros(n, bool), ~m
            tr = m & ~nulls
            return tr, nulls.copy(), ~(tr | nulls)
        parts = [tnf(ch) for ch in t[1]]
        if t[0] == "not":
            return parts[0][2], np.zeros(n, bool), parts[0][0]
        tr = np.ones(n, bool) if t[0] == "and" else np.zeros(n, bool)
        u = tr.copy()
        for ct, cn, _ in parts:
            tr = (tr & ct) if t[0] == "and" else (tr | ct)
            u = (u & (ct | cn)) if t[0] == "and" else (u | (ct | cn))
        return tr, np.zeros(n, bool), ~u
    return tnf(fq.tree)[0]


def aggregation_min(d):
    """MinAggregationFunction.aggregate (MinAggregationFunction.java:116-127): a fold of java.lang.Math.min from +Infinity -- NaN wins,
    -0.0 < 0.0."""
    if len(d) == 0:
        return math.inf
    if np.isnan(d).any():
        return math.nan
    m = float(d.min())
    return -0.0 if m == 0.0 and np.signbit(d[d == 0.0]).any() else m


def aggregation_max(d):
    """MaxAggregationFunction.aggregate (MaxAggregationFunction.java:116-127): Math.max from -Infinity -- NaN wins, 0.0 > -0.0."""
    if len(d) == 0:
        return -math.inf
    if np.isnan(d).any():
        return math.nan
    m = float(d.max())
    return (0.0 if (~np.signbit(d[d == 0.0])).any() else -0.0) if m == 0.0 else m


def group_min(d):
    """MinAggregationFunction.aggregateGroupBySV (MinAggregationFunction.java:180-186): `if (value < holder)` from +Infinity -- a NaN
    never enters, an all-NaN group keeps +Infinity.  (The sign of a zero minimum is the first zero's in doc order: not modelled.)"""
    d = d[~np.isnan(d)]
    return float(d.min()) if len(d) else math.inf


def group_max(d):
    """MaxAggregationFunction.aggregateGroupBySV (MaxAggregationFunction.java:180-186): `if (value > holder)` from -Infinity."""
    d = d[~np.isnan(d)]
    return float(d.max()) if len(d) else -math.inf


class ExpAgg:
    """What one aggregation returns: `count` values reached it; `isum` the exact integer sum (INT / LONG) or None; `fsum` the correctly
    rounded sum of the doubles (math.fsum; NaN / +-inf by IEEE rules) and `sumabs` = sum |x|; `min` / `max`."""
    __slots__ = ("count", "isum", "fsum", "sumabs", "min", "max", "pool")

    def __init__(self):
        self.count, self.isum, self.fsum, self.sumabs, self.min, self.max, self.pool = 0, None, None, 0.0, None, None, None


def exact_fp_sum(d):
    if np.isnan(d).any() or (np.isposinf(d).any() and np.isneginf(d).any()):
        return math.nan, math.inf
    if np.isinf(d).any():
        return (math.inf if np.isposinf(d).any() else -math.inf), math.inf
    try:
        return math.fsum(d.tolist()), math.fsum(np.abs(d).tolist())
    except OverflowError:            # several copies of the largest finite value (never next to -inf or its negative): +inf in any order
        return math.inf, math.inf


def _aggregate(seg, fq, function, column, docs, grouped):
    e = ExpAgg()
    if function == Q.COUNT and column < 0:
        e.count = len(docs)
        return e
    col = seg.cols[column]
    if fq.null_handling and col.nulls is not None:
        docs = docs[~col.nulls[docs]]             # NullableSingleInputAggregationFunction: the null docs of THIS column do not reach it
    e.count = len(docs)
    if function == Q.COUNT:
        return e
    e.pool = col.pool
    if function in (Q.SUM, Q.AVG):
        if col.is_fp:
            e.fsum, e.sumabs = exact_fp_sum(col.doubles()[docs])
        else:
            ints = [int(v) for v in col.values[docs].tolist()]
            e.isum, e.sumabs = sum(ints), float(sum(abs(v) for v in ints))
    elif function == Q.MIN:
        e.min = (group_min if grouped else aggregation_min)(col.doubles()[docs])
    else:
        e.max = (group_max if grouped else aggregation_max)(col.doubles()[docs])
    return e


class Expected:
    def __init__(self):
        self.mask, self.aggregations, self.groups, self.limit_reached = None, [], {}, False


def expected(seg, fq):
    """The exact model: what the query returns, from the columns' VALUES alone."""
    out = Expected()
    out.mask = filter_mask(seg, fq)
    docs = np.flatnonzero(out.mask)
    cols = seg.cols
    has_null_values = fq.null_handling and any(c >= 0 and cols[c].nulls is not None for _, c in fq.aggs)
    if not fq.group_by:
        # AggregationPlanNode.java:130-152 / NonScanBasedAggregationOperator: COUNT / MIN / MAX over dictionary columns of a query that
        # matches every doc are answered from the segment metadata and the dictionaries' first and last entries -- Double.compare order,
        # so MAX of a dictionary that holds NaN is NaN and its MIN is the first entry.
        t = fq.tree
        match_all = t is None or (t[0] == "leaf" and ((t[1].kind == "match_all" and not t[1].exclusive) or (t[1].kind == "match_none" and t[1].exclusive)))
        if match_all and not has_null_values and all(f == Q.COUNT or (f in (Q.MIN, Q.MAX) and cols[c].is_dict) for f, c in fq.aggs):
            for f, c in fq.aggs:
                e = ExpAgg()
                e.count = seg.n
                if f == Q.MIN:
                    e.min = float(cols[c].dict_values[0])
                if f == Q.MAX:
                    e.max = float(cols[c].dict_values[-1])
                out.aggregations.append(e)
            return out
        out.aggregations = [_aggregate(seg, fq, f, c, docs, False) for f, c in fq.aggs]
        return out
    # group keys: identity tuples; under null handling a null key value is a key of its own
    ident, product, no_dict, nullable = [], 1, False, has_null_values
    for g in fq.group_by:
        c = cols[g]
        card = c.key_scale()[2]
        null = c.nulls if (fq.null_handling and c.nulls is not None) else None
        idc = key_identity(c.values).copy()
        if null is not None:
            idc[null] = 0
            card += 1
            nullable = True
        ident += [idc, null.astype(np.int64) if null is not None else np.zeros(seg.n, np.int64)]
        product *= card
        no_dict |= not c.is_dict
    # DictionaryBasedGroupKeyGenerator.java:150-184, NoDictionary*GroupKeyGenerator :73-79: array based (every key) up to the threshold, unless
    # the no-dictionary generators run (a raw key column; null handling with nulls in a key or aggregated column): then, and above the
    # threshold, group ids go to the first min(product, numGroupsLimit) keys in docId order and the docs of later keys reach no holder.
    limit = fq.limit if fq.limit > 0 else DEFAULT_GROUPS_LIMIT
    map_based = product > ARRAY_BASED_THRESHOLD or nullable or no_dict
    rows = np.stack([x[docs] for x in ident], axis=1) if len(docs) else np.zeros((0, len(ident)), np.int64)
    uniq, first, inverse = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    by_first = np.argsort(first, kind="stable")
    keep = by_first[: min(product, limit)] if map_based else by_first
    out.limit_reached = bool(map_based and len(keep) >= limit)
    order = np.argsort(inverse, kind="stable")
    bounds = np.searchsorted(inverse[order], np.arange(len(uniq) + 1))
    for u in keep.tolist():
        gdocs = docs[order[bounds[u]: bounds[u + 1]]]
        key = tuple(None if uniq[u][2 * j + 1] else int(uniq[u][2 * j]) for j in range(len(fq.group_by)))
        out.groups[key] = [_aggregate(seg, fq, f, c, gdocs, True) for f, c in fq.aggs]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# a Result (the oracle's or the device's) against the model
# ------------------------------------------------------------------------------------------------------------------------------------
def result_keys(seg, fq, result):
    """The result's rows keyed like the model's groups: every digit of Result.group_keys turned into the key value's identity."""
    scales = [seg.cols[g].key_scale() for g in fq.group_by]
    out = {}
    for tup, vals in zip(result.group_keys, result.groups.values()):
        key = []
        for (how, ref, card), d in zip(scales, tup):
            if d == card:
                key.append(None)                  # the null digit (enableNullHandling)
            elif how == "offset":
                key.append(ref + d)
            elif how == "rank":
                key.append(int(ref[d]))
            else:
                key.append(int(key_identity(ref[d: d + 1])[0]))
        out[tuple(key)] = vals
    assert len(out) == len(result.group_keys), "two result rows with one key"
    return out


def fp_sum_bound(e):
    """count * 2^-53 * sum|x|: |a double sum in ANY order of its count - 1 additions - the exact sum| <= gamma_(n-1) * sum|x| with
    gamma_(n-1) = (n-1)u / (1 - (n-1)u) <= n u for these n, u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)."""
    return e.count * U * e.sumabs


def same_extreme(got, want, sign_too):
    if math.isnan(want):
        return math.isnan(got)
    return got == want and (not sign_too or want != 0.0 or math.copysign(1.0, got) == math.copysign(1.0, want))


def check_agg(v, e, function, grouped, where, fp_sums=True):
    """One AggValue against the model's ExpAgg.  fp_sums=False leaves FLOAT / DOUBLE sums out (callers that hold them to another yardstick)."""
    assert v.count == e.count, "%s: count %d, model %d" % (where, v.count, e.count)
    if function in (Q.SUM, Q.AVG):
        if e.isum is not None:
            assert v.sum_i64 == ((e.isum + 2 ** 63) % 2 ** 64) - 2 ** 63, "%s: integer sum %d, model %d" % (where, v.sum_i64, e.isum)
            assert (not v.sum_exact) or v.sum_i64 == e.isum, "%s: a wrapped sum flagged exact" % where
            assert abs(v.sum - float(e.isum)) <= fp_sum_bound(e) + abs(float(e.isum)) * U, "%s: sum %r, model %d" % (where, v.sum, e.isum)
        elif fp_sums:
            assert not v.sum_exact, "%s: a floating-point sum flagged exact" % where
            if math.isnan(e.fsum) or math.isinf(e.fsum):
                assert (math.isnan(v.sum) and math.isnan(e.fsum)) or v.sum == e.fsum, "%s: sum %r, model %r" % (where, v.sum, e.fsum)
            else:
                assert abs(v.sum - e.fsum) <= fp_sum_bound(e), "%s: sum %r, exact %r, off by %.3g, bound %.3g (%d values, sum|x| %.3g)" % (
                    where, v.sum, e.fsum, abs(v.sum - e.fsum), fp_sum_bound(e), e.count, e.sumabs)
    elif function == Q.MIN:
        assert same_extreme(v.min, e.min, not grouped), "%s: min %r, model %r" % (where, v.min, e.min)
    elif function == Q.MAX:
        assert same_extreme(v.max, e.max, not grouped), "%s: max %r, model %r" % (where, v.max, e.max)


def check_result(seg, fq, result, exp, fp_sums=True):
    """A whole Result against the model: docs scanned, groups by key, every aggregation."""
    assert result.stats[0] == int(exp.mask.sum()), "numDocsScanned %d, model %d" % (result.stats[0], int(exp.mask.sum()))
    assert result.stats[3] == seg.n
    if not fq.group_by:
        assert len(result.aggregations) == len(exp.aggregations)
        for i, (f, _) in enumerate(fq.aggs):
            check_agg(result.aggregations[i], exp.aggregations[i], f, False, "agg %d" % i, fp_sums)
        return
    rows = result_keys(seg, fq, result)
    assert sorted(rows, key=repr) == sorted(exp.groups, key=repr), "group keys differ: %d rows, model %d" % (len(rows), len(exp.groups))
    assert result.num_groups_limit_reached == exp.limit_reached
    for key, want in exp.groups.items():
        for i, (f, _) in enumerate(fq.aggs):
            check_agg(rows[key][i], want[i], f, True, "group %r agg %d" % (key, i), fp_sums)


def mask_words(mask):
    """A boolean doc mask as the 64-bit words pg_filter_bitmap returns."""
    n = len(mask)
    padded = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    padded[:n] = mask
    return np.packbits(padded, bitorder="little").view(np.uint64)


def coverage(segments_and_queries):
    """What a seed set exercises, as a Counter of labels (tests/test_fuzz_cases_cpu.py holds it to thresholds)."""
    from collections import Counter
    names = {Q.COUNT: "count", Q.SUM: "sum", Q.MIN: "min", Q.MAX: "max", Q.AVG: "avg"}
    c = Counter()
    for seg, queries in segments_and_queries:
        c["size:%d" % seg.n] += 1
        for fq in queries:
            c["null_handling:%s" % ("on" if fq.null_handling else "off")] += 1
            c["group_by:%d" % len(fq.group_by)] += 1
            leaves = fq.leaves()
            c["shared_pred"] += len(leaves) != len({id(x) for x in leaves})
            for leaf in {id(x): x for x in leaves}.values():
                c["leaf:" + leaf.kind] += 1
                if leaf.kind not in ("match_all", "match_none", "doc_range", "is_null"):
                    c["filter_column:" + seg.cols[leaf.column].kind] += 1
                if leaf.kind in ("raw_set", "raw_set_f64"):
                    distinct = len(set(leaf.args["values"]))
                    c["set_size:1"] += distinct == 1
                    c["set_size:cap"] += distinct == CAP
                    c["set_exclusive"] += leaf.exclusive
                if leaf.kind in ("raw_range", "raw_range_f64"):
                    c["range_lo_above_hi"] += leaf.args["lo"] > leaf.args["hi"]
            for f, col in fq.aggs:
                c["function:" + names[f]] += 1
                if col >= 0 and f != Q.COUNT:
                    cc = seg.cols[col]
                    c["aggregated_column:" + cc.kind] += 1
                    if cc.pool:
                        c["sum_pool:" + cc.pool] += f in (Q.SUM, Q.AVG)
                    for what in ("nan", "inf", "zero"):
                        c["aggregated_has:" + what] += cc.is_fp and cc.has(what)
                        c["group_min_max_has:" + what] += bool(fq.group_by) and f in (Q.MIN, Q.MAX) and cc.is_fp and cc.has(what)
                    c["min_max_dict_fp_nan"] += f in (Q.MIN, Q.MAX) and cc.is_fp and cc.is_dict and cc.has("nan")
            for g in fq.group_by:
                cc = seg.cols[g]
                c["key_column:" + cc.kind] += 1
                c["key_scale:" + cc.key_scale()[0]] += 1
                for what in ("nan", "inf", "zero"):
                    c["key_has:" + what] += cc.is_fp and cc.has(what)
            c["limit_set"] += fq.limit > 0
    return c
