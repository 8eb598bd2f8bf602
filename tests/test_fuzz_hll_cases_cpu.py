"""CPU tier of the DISTINCTCOUNTHLL fuzz (tests/fuzz_hll_cases.py): for every seed tests/test_gpu_fuzz_hll.py uses,
  * the derivation leaves the typed fuzz's and the value fuzz's random streams alone (segments, base queries and value queries are the same,
    object for object, in a second generation made after the HLL queries were derived) and is itself deterministic;
  * every derived query keeps the shape rules plan_distinct declines by (1-4 distinct slots, log2m of {8, 4, 12, 14}, one encoding, no
    nullable value column or key under null handling, DISTINCTCOUNT beside the HLLs on dictionary columns only and at most four distinct
    value columns, admitted keys only, the key product within numGroupsLimit, no wide raw range leaf, an ungrouped raw query's registers
    within the LDS budget less the set area a dict_set leaf stages);
  * the oracle answers EVERY companion query (HLL and DISTINCTCOUNT turned into COUNT(*), through the twin segment for doc sets) -- it
    declines nothing, which keeps the GPU test's decline cap honest -- and agrees with F.expected; oracle.filter_bitmap equals the model's
    mask bit for bit;
  * for every value aggregation and every group the numpy model's registers equal ph_hll_offer_longs over the same longs: the arithmetic of
    pinot_amd/csrc/pg_hll.h, which the kernels include, independent of the numpy restatement;
  * the share of derived queries a size message can reach at these cardinalities stays within the GPU test's decline cap.
The last test holds the derivation to what it is meant to cover, so that it cannot narrow unnoticed."""
import numpy as np
import pytest

import fuzz_cases as F
import fuzz_hll_cases as FH
import fuzz_value_cases as V
import hll_cases as HL
from oracle import oracle
from pinot_amd import host
from pinot_amd import query as Q
from test_gpu_fuzz_typed import MAX_DECLINED

_CACHE = {}


def generated(seed):
    if seed not in _CACHE:
        seg = F.make_segment(seed)
        queries = F.make_queries(seg)
        _CACHE[seed] = (seg, queries, FH.make_hll_queries(seg, queries))
    return _CACHE[seed]


def _typed(q):
    return (q.aggs, q.group_by, q.null_handling, q.limit, [x.kind for x in q.leaves()])


def _value(v):
    return (v.base_index, v.family, v.raw, v.aggs, v.group_by, v.valid_format, None if v.valid is None else int(v.valid.sum()), v.variant)


def _hll(h):
    return (h.base_index, h.raw, h.aggs, h.slots, h.group_by, h.valid_format, None if h.valid is None else h.valid.tobytes(), h.variant)


def test_the_typed_and_the_value_fuzz_are_what_they_were_and_the_derivation_is_deterministic():
    for seed in (0, 7, 23):
        # first generation: nothing of this module has run for the segment yet
        seg = F.make_segment(seed)
        queries = F.make_queries(seg)
        values = V.make_value_queries(seg, queries)
        hqs = FH.make_hll_queries(seg, queries)
        # second generation, after the HLL derivation
        again = F.make_segment(seed)
        assert again.n == seg.n and [c.kind for c in again.cols] == [c.kind for c in seg.cols]
        assert all(np.array_equal(a.values, b.values, equal_nan=a.is_fp) for a, b in zip(again.cols, seg.cols))
        requeried = F.make_queries(again)
        assert [_typed(q) for q in requeried] == [_typed(q) for q in queries]
        assert [_value(v) for v in V.make_value_queries(again, requeried)] == [_value(v) for v in values]
        assert [_hll(h) for h in FH.make_hll_queries(again, requeried)] == [_hll(h) for h in hqs]
        assert [_hll(h) for h in generated(seed)[2]] == [_hll(h) for h in hqs]
    assert FH.SALT != V.SALT


@pytest.mark.parametrize("seed", F.SEEDS)
def test_derived_queries_keep_the_shape_rules_and_the_oracle_answers_every_companion(seed):
    seg, queries, hqs = generated(seed)
    for hq in hqs:
        where = "seed %d %s" % (seed, hq.describe(seg))
        base = queries[hq.base_index]
        # shape
        assert hq.tree is base.tree and hq.null_handling == base.null_handling and V.eligible(seg, base), where
        assert 1 <= len(hq.slots) <= FH.MAX_SLOTS and all(log2m in (8, 4, 12, 14) for _, log2m in hq.slots), where
        assert all(Q.is_hll(f) or f in (Q.DISTINCTCOUNT, Q.COUNT, Q.SUM, Q.MIN, Q.MAX, Q.AVG) for f, _ in hq.aggs) and hq.hll_positions, where
        assert len(hq.value_columns) <= FH.MAX_SLOTS, where
        assert not (hq.raw and hq.distinct_positions) and len(hq.distinct_positions) <= 1, where
        for c in hq.value_columns:
            assert seg.cols[c].is_dict != hq.raw and not (hq.null_handling and seg.cols[c].nulls is not None), where
        assert len(hq.group_by) <= V.MAX_KEYS, where
        for g in hq.group_by:
            assert (seg.cols[g].is_dict or seg.cols[g].key_scale()[0] == "offset") and not (hq.null_handling and seg.cols[g].nulls is not None), where
        if hq.group_by:
            assert FH.key_product(seg, hq.group_by) <= (hq.limit if hq.limit > 0 else F.DEFAULT_GROUPS_LIMIT), where
        elif hq.raw:
            has_set = any(x.kind == "dict_set" for x in hq.leaves())
            assert FH.register_bytes(hq.slots) + (FH.SET_AREA if has_set else 0) <= FH.LDS_BUDGET == 159744, where
        if hq.valid is not None:
            assert hq.valid.shape == (seg.n,) and hq.valid_format in ("words", "roaring"), where
        # the oracle on the companion (raises on a decline: there is none), the exact model of the ordinary fields, the masks
        twin, tfq = hq.twin(seg)
        try:
            assert not any(FH.is_value_function(f) for f, _ in tfq.aggs)
            want = oracle.execute(twin.data, tfq.spec)
            exp = F.expected(twin, tfq)
            F.check_result(twin, tfq, want, exp)
            mask = V.model_mask(seg, hq)
            assert np.array_equal(mask, exp.mask), "the user's part AND the valid mask is not the twin's filter"
            if tfq.tree is not None:
                words, card = oracle.filter_bitmap(twin.data, tfq.spec)
                assert card == int(mask.sum()) and np.array_equal(words, F.mask_words(mask)), "oracle.filter_bitmap differs from the model's mask"
            # the model's registers against the header the kernels include
            m = FH.model(seg, hq, mask)
            lists = m.lists if hq.group_by else {(): m.lists}
            docs_of = m.docs if hq.group_by else {(): m.docs}
            if hq.group_by:
                assert sorted(lists, key=repr) == sorted(exp.groups, key=repr), "the HLL model's groups are not F.expected's"
            assert sum(len(d) for d in docs_of.values()) == int(mask.sum())
            for key, per in lists.items():
                for a, listed in per.items():
                    f, c = hq.aggs[a]
                    col = seg.cols[c]
                    if f == Q.DISTINCTCOUNT:
                        assert len(listed) == (col.cardinality if m.whole_dictionary else len(np.unique(col.ids[docs_of[key]])))
                        continue
                    dtype = FH.stored_dtype(col)
                    assert col.values.dtype == dtype and (not col.is_dict or np.asarray(col.dict_values).dtype == dtype)
                    offered = np.asarray(col.dict_values) if m.whole_dictionary else col.values[docs_of[key]]
                    longs = HL.longs_of(offered, dtype)
                    log2m = Q.hll_log2m(f)
                    assert listed.shape == (1 << log2m,) and np.array_equal(listed, host.hll_offer_longs(longs, log2m)), "registers of agg %d group %r" % (a, key)
                    assert int(np.count_nonzero(listed)) <= len(np.unique(longs))
        except AssertionError as e:
            raise AssertionError("%s: %s" % (where, e)) from e


def test_the_size_messages_reach_no_more_queries_than_the_decline_cap_allows():
    """Per half of the seed set (a GPU case), the derived queries whose register or bit matrices exceed their cap at these cardinalities."""
    for half in (0, 1):
        hqs = [(generated(seed)[0], h) for seed in F.SEEDS[half::2] for h in generated(seed)[2]]
        reached = [FH.size_declines(seg, h) for seg, h in hqs]
        count = sum(r is not None for r in reached)
        print("half %d: %d derived, size messages can reach %d (%r)" % (half, len(hqs), count, sorted({r for r in reached if r})))
        assert count <= MAX_DECLINED * len(hqs), "the size messages alone may take %d of %d derived queries" % (count, len(hqs))


# Coverage of the committed seed set (PINOT_FUZZ_SEED_BASE=0): what the seeds produce, measured; each label is held to half of its figure.
MEASURED = {
    "derived": 341, "distinctcount_beside:no": 283, "distinctcount_beside:other_column": 32, "distinctcount_beside:same_column": 26, "doc_set:none":
    231, "doc_set:roaring": 48, "doc_set:words": 62, "doc_set_density:empty": 21, "doc_set_density:full": 24, "doc_set_density:partial": 65,
    "encoding:dict_double": 63, "encoding:dict_float": 65, "encoding:dict_int": 269, "encoding:dict_long": 41, "encoding:raw_double": 93,
    "encoding:raw_float": 80, "encoding:raw_int": 126, "encoding:raw_long": 115, "extras": 150, "function:DISTINCTCOUNT": 58,
    "function:DISTINCTCOUNTHLL": 942, "grouped:dict": 69, "grouped:no": 207, "grouped:raw": 65, "grouped:yes": 134, "inverted_leaf": 34,
    "key_scale:dict": 136, "key_scale:offset": 7, "keys:0": 207, "keys:1": 125, "keys:2": 9, "lds_room_with_set_area": 19, "leaf:dict_range": 116,
    "leaf:dict_set": 94, "leaf:doc_range": 35, "leaf:inverted_range": 22, "leaf:inverted_set": 16, "leaf:is_null": 20, "leaf:match_all": 19,
    "leaf:match_none": 26, "leaf:raw_range": 64, "leaf:raw_set": 63, "leaf:raw_set_f64": 47, "leaves:0": 54, "leaves:1": 179, "leaves:2": 37,
    "leaves:3+": 71, "log2m:12": 225, "log2m:14": 201, "log2m:4": 227, "log2m:8": 199, "null_handling:off": 271, "null_handling:on": 70,
    "pass_alone:dict": 60, "pass_alone:no": 233, "pass_alone:raw": 48, "pass_alone:yes": 108, "plain_enumerator": 171, "same_column_two_log2m": 186,
    "same_slot_twice": 90, "shared_pred": 23, "size_decline_possible": 1, "slots:1": 88, "slots:2": 73, "slots:3": 102, "slots:4": 78,
    "value_has:inf": 92, "value_has:nan": 51, "value_has:zero": 180, "variant:base": 248, "variant:small-key": 93, "whole_dictionary": 6,
}
COVERAGE_THRESHOLDS = {label: max(1, figure // 2) for label, figure in MEASURED.items()}
REQUIRED_LABELS = ["function:DISTINCTCOUNTHLL", "function:DISTINCTCOUNT", "encoding:dict_int", "encoding:dict_long", "encoding:dict_float", "encoding:dict_double",
                   "encoding:raw_int", "encoding:raw_long", "encoding:raw_float", "encoding:raw_double", "log2m:4", "log2m:8", "log2m:12", "log2m:14",
                   "slots:1", "slots:2", "slots:3", "slots:4", "same_column_two_log2m", "distinctcount_beside:same_column", "distinctcount_beside:other_column",
                   "grouped:yes", "grouped:no", "key_scale:dict", "key_scale:offset", "doc_set:words", "doc_set:roaring", "doc_set_density:empty",
                   "doc_set_density:full", "doc_set_density:partial", "leaf:dict_range", "leaf:dict_set", "leaf:doc_range", "leaf:inverted_range", "leaf:inverted_set",
                   "leaf:is_null", "leaf:match_all", "leaf:match_none", "leaf:raw_range", "leaf:raw_set", "leaf:raw_set_f64", "null_handling:on", "null_handling:off",
                   "pass_alone:raw", "pass_alone:dict", "whole_dictionary", "value_has:nan", "value_has:inf", "value_has:zero"]


def test_the_derivation_covers_what_it_is_meant_to():
    if F.SEED_BASE != 0:
        return                  # a soak over other seeds: the thresholds are those of the committed seed set
    c = FH.coverage((generated(seed)[0], generated(seed)[2]) for seed in F.SEEDS)
    assert all(label in MEASURED and MEASURED[label] > 0 for label in REQUIRED_LABELS), [label for label in REQUIRED_LABELS if not MEASURED.get(label)]
    short = {k: (c[k], need) for k, need in COVERAGE_THRESHOLDS.items() if c[k] < need}
    assert not short, "the derivation narrowed: %r" % short
    assert len(COVERAGE_THRESHOLDS) >= 50
    assert c["grouped:yes"] >= 40 and c["grouped:raw"] >= 20 and c["grouped:dict"] >= 20
