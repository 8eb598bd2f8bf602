"""DISTINCTCOUNTHLL queries derived from the typed fuzz (tests/fuzz_cases.py) the way tests/fuzz_value_cases.py derives DISTINCTCOUNT / PERCENTILE
queries, and an EXACT MODEL of what each returns -- shared by tests/test_fuzz_hll_cases_cpu.py and tests/test_gpu_fuzz_hll.py.  Nothing here needs
a GPU or the oracle.  Deterministic in (seed, PINOT_FUZZ_SEED_BASE).

Neither the typed fuzz's nor the value fuzz's random stream is touched: every choice made here comes from a generator of its own,
np.random.default_rng([seed, SEED_BASE, SALT]) with a salt of this module.  The filter, keys, extras, COUNT(*), doc sets and key repair are
fuzz_value_cases' (V.eligible, V.repaired_keys, V._extra_ok, the twin machinery of V.ValueQuery); what differs:
  * 1-4 distinct SLOTS (column, log2m), log2m from {the plain enumerator (8), 4, 12, 14}; about a third of the queries with two slots or more
    put the same column under two log2m; about a quarter repeat one slot as a further aggregation (log2m 8 then in its other spelling,
    PG_AGG_HLL(8)): two aggregations of one slot must return the same bytes;
  * all slots raw or all dictionary (the engine declines a mix), no value column with a null vector under null handling;
  * on dictionary columns about a third of the queries carry a DISTINCTCOUNT too, on one of the HLL columns (two users of one bitset) or on
    another dictionary column while the query has fewer than four; never on raw columns (the engine declines that);
  * an ungrouped raw query keeps sum(4 << log2m) within the LDS budget, less the staged set area when the tree has a dict_set leaf: the
    largest slot is dropped until it fits, so that shape alone declines nothing;
  * under GROUP BY the DATA may still decline a query by size: "register matrices of N bytes exceed ..." (key product x 4 << log2m per
    slot above PG_HLL_GROUP_MAX_BYTES) and the DISTINCTCOUNT's "bit matrices of N bytes exceed ..."; size_declines restates the arithmetic
    and the CPU tier counts whom it reaches (1 of 341 derived queries at the committed seeds).

The model: registers = hll_cases.registers over the model mask's docs, the values AS STORED in the column's own dtype (a FLOAT dictionary entry is
its 32 stored bits); per group keyed as V.model keys them.  A dictionary-column query the reference answers without a scan
(AggregationPlanNode.java:98-115, DISTINCTCOUNTHLL among DICTIONARY_BASED_FUNCTIONS: the filter matches everything, every function is COUNT,
DISTINCTCOUNT, DISTINCTCOUNTHLL or a dictionary MIN / MAX, no aggregation argument has null values under null handling) is the registers of
the WHOLE dictionary, with statistics (docs, 0, 0, docs).  numEntriesScannedPostFilter is docs x the distinct columns the ORIGINAL query projects."""
import itertools

import numpy as np

import doc_set_cases as D
import fuzz_cases as F
import fuzz_value_cases as V
import hll_cases as HL
from pinot_amd import _abi
from pinot_amd import query as Q

SALT = 0x484C4C
LOG2MS = (0, 4, 12, 14)                                                  # 0: the plain enumerator, which means log2m 8
MAX_SLOTS = 4                                                            # kMaxAggCols
LDS_BUDGET = _abi.PG_DISTINCT_LDS_MAX_DICT_IDS // 8                      # kLdsBudget
SET_AREA = _abi.PG_STAGED_SET_LDS_WORDS * 4                              # kSetLdsWords words
GROUP_MAX_BYTES = _abi.PG_HLL_GROUP_MAX_BYTES
SIZE_DECLINES = [r"DISTINCTCOUNTHLL register matrices of \d+ bytes exceed", r"DISTINCTCOUNT bit matrices of \d+ bytes exceed"]


def function_word(log2m):
    return Q.DISTINCTCOUNTHLL if log2m == 0 else Q.hll(log2m)


def is_value_function(f):
    return Q.is_hll(f) or f == Q.DISTINCTCOUNT


class HllQuery(V.ValueQuery):
    """One derived query (V.ValueQuery's fields and twin machinery).  The value positions are the HLL aggregations AND the DISTINCTCOUNT
    beside them: the companion query turns both into COUNT(*)."""

    def __init__(self, base_index, raw, aggs, tree, group_by, null_handling, limit, valid, valid_format, variant):
        V.ValueQuery.__init__(self, base_index, Q.DISTINCTCOUNTHLL, raw, aggs, tree, group_by, null_handling, limit, valid, valid_format, variant)
        self.hll_positions = [a for a, (f, _) in enumerate(aggs) if Q.is_hll(f)]
        self.distinct_positions = [a for a, (f, _) in enumerate(aggs) if f == Q.DISTINCTCOUNT]
        self.value_positions = sorted(self.hll_positions + self.distinct_positions)
        self.value_columns = list(dict.fromkeys(aggs[a][1] for a in self.value_positions))
        self.slots = list(dict.fromkeys((aggs[a][1], Q.hll_log2m(aggs[a][0])) for a in self.hll_positions))
        self.companion_aggs = [((Q.COUNT, -1) if is_value_function(f) else (f, c)) for f, c in aggs]
        self.companion = F.FuzzQuery(self.companion_aggs, tree, group_by, null_handling, limit)
        self.counts_only = all(is_value_function(f) or (f == Q.COUNT and (c < 0 or not null_handling)) for f, c in aggs)

    def describe(self, seg):
        name = lambda f: "HLL%d" % Q.hll_log2m(f) if Q.is_hll(f) else f
        return "base query %d %s (DISTINCTCOUNTHLL %s, n=%d, aggs=%r, group_by=%r, null_handling=%r, limit=%d, leaves=%r, doc set %s)" % (
            self.base_index, self.variant, "raw" if self.raw else "dictionary", seg.n,
            [(name(f), seg.cols[c].kind if c >= 0 else "*") for f, c in self.aggs], [seg.cols[k].kind for k in self.group_by], self.null_handling, self.limit,
            [x.kind for x in self.leaves()], "none" if self.valid is None else "%s %d docs" % (self.valid_format, int(self.valid.sum())))


# ------------------------------------------------------------------------------------------------------------------------------------
# derivation
# ------------------------------------------------------------------------------------------------------------------------------------
def register_bytes(slots):
    return sum(4 << log2m for _, log2m in slots)


def key_product(seg, keys):
    return int(np.prod([seg.cols[g].key_scale()[2] for g in keys], dtype=object)) if keys else 1


def lds_room(fq):
    """What an ungrouped raw query's registers may take: the budget, less the set area a dict_set leaf stages beside them."""
    return LDS_BUDGET - (SET_AREA if any(x.kind == "dict_set" for x in fq.leaves()) else 0)


def _derive_one(rng, counter, seg, fq, base_index, keys, variant):
    cols = seg.cols
    nh = fq.null_handling
    candidates = {raw: [i for i, c in enumerate(cols) if c.is_dict != raw and not (nh and c.nulls is not None)] for raw in (False, True)}
    encodings = [raw for raw in (False, True) if candidates[raw]]
    if not encodings:
        return None
    raw = encodings[int(rng.integers(0, len(encodings)))]
    pool = candidates[raw]
    want = int(rng.integers(1, MAX_SLOTS + 1))
    slots = []
    twice = want >= 2 and rng.integers(0, 3) == 0
    for _ in range(4 * MAX_SLOTS):
        if len(slots) == want:
            break
        column = slots[0][0] if (twice and len(slots) == 1) else pool[int(rng.integers(0, len(pool)))]
        slot = (int(column), Q.hll_log2m(function_word(LOG2MS[int(rng.integers(0, len(LOG2MS)))])))
        if slot not in slots:
            slots.append(slot)
    # the room a query's shape has: the ungrouped raw pass keeps every slot's registers in LDS (the smallest slot always fits)
    while raw and not keys and register_bytes(slots) > lds_room(fq):
        slots.remove(max(slots, key=lambda s: s[1]))
    aggs = [(Q.DISTINCTCOUNTHLL if log2m == 8 else Q.hll(log2m), c) for c, log2m in slots]
    if rng.integers(0, 4) == 0:
        c, log2m = slots[int(rng.integers(0, len(slots)))]
        aggs.append((Q.hll(log2m), c))                                   # (log2m 8: the other spelling of the same slot)
    if not raw and rng.integers(0, 3) == 0:
        columns = list(dict.fromkeys(c for c, _ in slots))
        others = [c for c in pool if c not in columns]
        if others and len(columns) < MAX_SLOTS and rng.integers(0, 2):
            aggs.append((Q.DISTINCTCOUNT, int(others[int(rng.integers(0, len(others)))])))
        else:
            aggs.append((Q.DISTINCTCOUNT, int(columns[int(rng.integers(0, len(columns)))])))
    extras = []
    if rng.integers(0, 2):
        agg_cols = []
        for f, c in fq.aggs:
            if not V._extra_ok(seg, f, c, bool(keys), nh):
                continue
            if c >= 0 and f != Q.COUNT and c not in agg_cols:
                if not keys and len(agg_cols) >= F.MAX_AGG_COLUMNS:
                    continue
                agg_cols.append(c)
            extras.append((f, c))
    if extras:
        aggs = aggs + extras
        aggs = [aggs[i] for i in rng.permutation(len(aggs))]
    elif rng.integers(0, 2):
        aggs = aggs + [(Q.COUNT, -1)]
    valid = fmt = None
    if rng.integers(0, 3) == 0 and len(fq.leaves()) < F.MAX_LEAVES:
        valid = D.random_mask(rng, seg.n, float(rng.choice(V.VALID_DENSITIES)))
        fmt = ("words", "roaring")[next(counter) % 2]
    return HllQuery(base_index, raw, aggs, fq.tree, list(keys), nh, fq.limit if keys else 0, valid, fmt, variant)


def derive(seg, fq, rng, counter=None, base_index=-1):
    """Zero, one or two HLL queries of one base FuzzQuery."""
    counter = itertools.count() if counter is None else counter
    if not V.eligible(seg, fq):
        return []
    out = [_derive_one(rng, counter, seg, fq, base_index, V.repaired_keys(seg, fq), "base")]
    if not fq.group_by:
        small = [i for i, c in enumerate(seg.cols) if c.is_dict and c.cardinality <= V.SMALL_KEY and not (fq.null_handling and c.nulls is not None)]
        if small and rng.integers(0, 2):
            out.append(_derive_one(rng, counter, seg, fq, base_index, [small[int(rng.integers(0, len(small)))]], "small-key"))
    return [h for h in out if h is not None]


def make_hll_queries(seg, queries):
    """Every derived query of a fuzz segment, in base-query order."""
    rng = np.random.default_rng([seg.seed, F.SEED_BASE, SALT])
    counter = itertools.count()
    out = []
    for bi, fq in enumerate(queries):
        out += derive(seg, fq, rng, counter, bi)
    return out


def size_declines(seg, hq):
    """Which size message the DATA can raise for this query at the segment's cardinalities (plan_distinct's arithmetic restated), or None."""
    if not hq.group_by:
        return None
    product = key_product(seg, hq.group_by)
    if product * register_bytes(hq.slots) > GROUP_MAX_BYTES:
        return "register matrices"
    if not hq.raw:
        # (the room behind the last row -- at most 2^bits words of one column -- is left out: it decides nothing at these cardinalities)
        matrix = sum(product * ((seg.cols[c].cardinality + 31) // 32) * 4 for c in hq.value_columns)
        if matrix > _abi.PG_DISTINCT_GROUP_MAX_BYTES:
            return "bit matrices"
    return None


# ------------------------------------------------------------------------------------------------------------------------------------
# the exact model
# ------------------------------------------------------------------------------------------------------------------------------------
def from_dictionary(seg, hq):
    """V.from_dictionary's rule with DISTINCTCOUNTHLL among DICTIONARY_BASED_FUNCTIONS."""
    if hq.raw or hq.group_by or hq.valid is not None:
        return False
    t = hq.tree
    if not (t is None or (t[0] == "leaf" and ((t[1].kind == "match_all" and not t[1].exclusive) or (t[1].kind == "match_none" and t[1].exclusive)))):
        return False
    if hq.null_handling and any(c >= 0 and seg.cols[c].nulls is not None for _, c in hq.aggs):
        return False
    return all(f == Q.COUNT or is_value_function(f) or (f in (Q.MIN, Q.MAX) and seg.cols[c].is_dict) for f, c in hq.aggs)


def stored_dtype(col):
    return np.dtype(F.DTYPES[col.kind])


class HllModel:
    """`lists`: {aggregation index: want} or -- GROUP BY -- {key identity tuple: {aggregation index: want}}; want: uint8 registers of an HLL
    aggregation, sorted int32 dictIds of a DISTINCTCOUNT; `docs`: the same shape, the docs that reached the aggregations."""

    def __init__(self):
        self.mask, self.lists, self.docs, self.whole_dictionary = None, {}, {}, False


def _one(col, f, docs, whole):
    if f == Q.DISTINCTCOUNT:
        return np.arange(col.cardinality, dtype=np.int32) if whole else np.unique(col.ids[docs]).astype(np.int32)
    values = np.asarray(col.dict_values, dtype=stored_dtype(col)) if whole else np.ascontiguousarray(col.values[docs], dtype=stored_dtype(col))
    return HL.registers(values, stored_dtype(col), Q.hll_log2m(f))


def model(seg, hq, mask=None):
    out = HllModel()
    out.mask = V.model_mask(seg, hq) if mask is None else mask
    docs = np.flatnonzero(out.mask)
    out.whole_dictionary = from_dictionary(seg, hq)
    per = lambda d: {a: _one(seg.cols[hq.aggs[a][1]], hq.aggs[a][0], d, out.whole_dictionary) for a in hq.value_positions}
    if not hq.group_by:
        out.lists, out.docs = per(docs), docs
        return out
    ident = [F.key_identity(seg.cols[g].values)[docs] for g in hq.group_by]
    rows = np.stack(ident, axis=1) if len(docs) else np.zeros((0, len(ident)), np.int64)
    uniq, inverse = np.unique(rows, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    order = np.argsort(inverse, kind="stable")
    bounds = np.searchsorted(inverse[order], np.arange(len(uniq) + 1))
    for u in range(len(uniq)):
        key = tuple(int(x) for x in uniq[u])
        out.docs[key] = docs[order[bounds[u]: bounds[u + 1]]]
        out.lists[key] = per(out.docs[key])
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# a device Result against the model
# ------------------------------------------------------------------------------------------------------------------------------------
def check_values(seg, hq, result, m, where=""):
    """Every value aggregation of the result against the model -- registers through hll_cases.assert_one_register_set, a DISTINCTCOUNT's
    set through V.check_value -- the group set, and: two aggregations of one (column, log2m) hold identical bytes."""
    rows = V.result_rows(seg, hq, result)
    lists = m.lists if hq.group_by else {(): m.lists}
    assert sorted(rows, key=repr) == sorted(lists, key=repr), "%s: groups differ (%d rows, model %d)" % (where, len(rows), len(lists))
    for key, per in lists.items():
        first = {}
        for a, want in per.items():
            at = "%s group %r agg %d" % (where, key, a)
            v = rows[key][a]
            f, c = hq.aggs[a]
            if f == Q.DISTINCTCOUNT:
                V.check_value(v, want, Q.DISTINCTCOUNT, False, at)
                assert v.hll_registers is None, "%s: registers beside a set" % at
                continue
            HL.assert_one_register_set(v, want, at)
            assert v.dict_ids is None and v.dict_id_counts is None and v.value_counts is None, "%s: a list beside the registers" % at
            slot = (c, Q.hll_log2m(f))
            if slot in first:
                assert bytes(v.hll_registers) == bytes(rows[key][first[slot]].hll_registers), "%s: not the bytes of aggregation %d of the same slot" % (at, first[slot])
            first.setdefault(slot, a)
        for a, (f, _) in enumerate(hq.aggs):
            if not is_value_function(f):
                v = rows[key][a]
                assert v.dict_ids is None and v.dict_id_counts is None and v.value_counts is None and v.hll_registers is None, "%s: a list beside an ordinary function" % where


def same_results(one, other, hq):
    """Two device results of one query: identical registers, sets, ordinary fields and statistics (V.same_value_lists and the registers)."""
    V.same_value_lists(one, other, hq)
    rows = [(one.aggregations, other.aggregations)] if not hq.group_by else [(one.groups[g], other.groups[g]) for g in one.groups]
    for ra, rb in rows:
        for a in hq.hll_positions:
            assert bytes(ra[a].hll_registers) == bytes(rb[a].hll_registers), "the registers of aggregation %d differ" % a


# ------------------------------------------------------------------------------------------------------------------------------------
# coverage
# ------------------------------------------------------------------------------------------------------------------------------------
def coverage(segments_and_queries):
    """What a seed set's derived queries exercise, as a Counter of labels (tests/test_fuzz_hll_cases_cpu.py holds it to thresholds)."""
    from collections import Counter
    c = Counter()
    for seg, hqs in segments_and_queries:
        for hq in hqs:
            alone = hq.counts_only and not hq.group_by
            c["derived"] += 1
            c["function:DISTINCTCOUNTHLL"] += len(hq.hll_positions)
            c["function:DISTINCTCOUNT"] += len(hq.distinct_positions)
            c["slots:%d" % len(hq.slots)] += 1
            c["same_column_two_log2m"] += len({col for col, _ in hq.slots}) < len(hq.slots)
            c["same_slot_twice"] += len(hq.hll_positions) > len(hq.slots)
            c["distinctcount_beside:%s" % ("no" if not hq.distinct_positions else
                                           ("same_column" if hq.aggs[hq.distinct_positions[0]][1] in {col for col, _ in hq.slots} else "other_column"))] += 1
            for col, log2m in hq.slots:
                c["log2m:%d" % log2m] += 1
                c["encoding:" + seg.cols[col].kind] += 1
                for what in ("nan", "inf", "zero"):
                    c["value_has:" + what] += seg.cols[col].is_fp and seg.cols[col].has(what)
            c["plain_enumerator"] += any(hq.aggs[a][0] == Q.DISTINCTCOUNTHLL for a in hq.hll_positions)
            c["grouped:%s" % ("yes" if hq.group_by else "no")] += 1
            c["grouped:%s" % ("raw" if hq.raw else "dict")] += bool(hq.group_by)
            c["keys:%d" % len(hq.group_by)] += 1
            c["variant:" + hq.variant] += 1
            for g in hq.group_by:
                c["key_scale:" + seg.cols[g].key_scale()[0]] += 1
            c["pass_alone:%s" % ("yes" if alone else "no")] += 1
            c["pass_alone:%s" % ("raw" if hq.raw else "dict")] += alone
            c["null_handling:%s" % ("on" if hq.null_handling else "off")] += 1
            c["doc_set:%s" % (hq.valid_format or "none")] += 1
            if hq.valid is not None:
                c["doc_set_density:%s" % ("empty" if not hq.valid.any() else ("full" if hq.valid.all() else "partial"))] += 1
            c["whole_dictionary"] += from_dictionary(seg, hq)
            c["size_decline_possible"] += size_declines(seg, hq) is not None
            c["lds_room_with_set_area"] += hq.raw and not hq.group_by and any(x.kind == "dict_set" for x in hq.leaves())
            leaves = list({id(x): x for x in hq.leaves()}.values())
            c["leaves:%s" % ("0" if not leaves else ("1" if len(hq.leaves()) == 1 else ("2" if len(hq.leaves()) == 2 else "3+")))] += 1
            c["shared_pred"] += len(hq.leaves()) != len(leaves)
            for leaf in leaves:
                c["leaf:" + leaf.kind] += 1
            c["inverted_leaf"] += any(x.kind in ("inverted_range", "inverted_set") for x in leaves)
            c["extras"] += any(not is_value_function(f) and not (f == Q.COUNT and col < 0) for f, col in hq.aggs)
    return c
