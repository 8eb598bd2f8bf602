"""CPU tier of the value-function fuzz (tests/fuzz_value_cases.py): for every seed tests/test_gpu_fuzz_values.py uses,
  * the derivation leaves the typed fuzz's random stream alone (the segments and base queries are those of tests/fuzz_cases.py, object for
    object in a second generation) and is itself deterministic;
  * every derived query keeps the shape rules plan_distinct / plan_percentile decline by (one family, one encoding, 1-4 value columns, no
    nullable value column or key under null handling, admitted keys only, the key product within numGroupsLimit, no wide raw range leaf);
  * the oracle answers EVERY companion query (value functions turned into COUNT(*)) -- it declines nothing, which keeps the GPU test's
    decline cap honest -- and agrees with the exact model on the ordinary fields (F.check_result);
  * oracle.filter_bitmap equals the model's mask bit for bit.  Doc-set queries use the TWIN-SEGMENT trick of tests/doc_set_cases.py: the oracle
    and F.expected evaluate AND(user filter, inverted `= 1` leaf on a synthetic column); the model's own mask is F.filter_mask of the user's
    part AND the valid mask, and the two routes must give the same docs;
  * the model's lists are self-consistent (counts add up to the docs, the final percentiles are those of a plain sort).
The last test holds the derivation to what it is meant to cover, so that it cannot narrow unnoticed."""
import numpy as np
import pytest

import fuzz_cases as F
import fuzz_value_cases as V
import raw_value_cases as RV
from oracle import oracle
from pinot_amd import query as Q

_CACHE = {}


def generated(seed):
    if seed not in _CACHE:
        seg = F.make_segment(seed)
        queries = F.make_queries(seg)
        _CACHE[seed] = (seg, queries, V.make_value_queries(seg, queries))
    return _CACHE[seed]


def test_the_typed_fuzz_is_what_it_was_and_the_derivation_is_deterministic():
    for seed in (0, 7, 23):
        seg, queries, vqs = generated(seed)
        again = F.make_segment(seed)
        assert again.n == seg.n and [c.kind for c in again.cols] == [c.kind for c in seg.cols]
        assert all(np.array_equal(a.values, b.values, equal_nan=a.is_fp) for a, b in zip(again.cols, seg.cols))
        requeried = F.make_queries(again)
        assert [(q.aggs, q.group_by, q.null_handling, q.limit, [x.kind for x in q.leaves()]) for q in requeried] == \
               [(q.aggs, q.group_by, q.null_handling, q.limit, [x.kind for x in q.leaves()]) for q in queries]
        rederived = V.make_value_queries(again, requeried)
        assert [(v.base_index, v.family, v.raw, v.aggs, v.group_by, v.valid_format, None if v.valid is None else int(v.valid.sum())) for v in rederived] == \
               [(v.base_index, v.family, v.raw, v.aggs, v.group_by, v.valid_format, None if v.valid is None else int(v.valid.sum())) for v in vqs]


@pytest.mark.parametrize("seed", F.SEEDS)
def test_derived_queries_keep_the_shape_rules_and_the_oracle_answers_every_companion(seed):
    seg, queries, vqs = generated(seed)
    for vq in vqs:
        where = "seed %d %s" % (seed, vq.describe(seg))
        base = queries[vq.base_index]
        # shape
        assert vq.tree is base.tree and vq.null_handling == base.null_handling and V.eligible(seg, base), where
        families = {f for f, _ in vq.aggs if f in V.VALUE_FUNCTIONS}
        assert families == {vq.family} and 1 <= len(vq.value_columns) <= V.MAX_VALUE_COLUMNS, where
        assert len(vq.value_columns) == len(vq.value_positions), where
        for c in vq.value_columns:
            assert seg.cols[c].is_dict != vq.raw and not (vq.null_handling and seg.cols[c].nulls is not None), where
        assert len(vq.group_by) <= V.MAX_KEYS, where
        for g in vq.group_by:
            assert (seg.cols[g].is_dict or seg.cols[g].key_scale()[0] == "offset") and not (vq.null_handling and seg.cols[g].nulls is not None), where
        if vq.group_by:
            product = int(np.prod([seg.cols[g].key_scale()[2] for g in vq.group_by], dtype=object))
            assert product <= (vq.limit if vq.limit > 0 else F.DEFAULT_GROUPS_LIMIT), where
        if vq.valid is not None:
            assert vq.valid.shape == (seg.n,) and vq.valid_format in ("words", "roaring"), where
        # the oracle on the companion (raises on a decline: there is none), the exact model of the ordinary fields, the masks
        twin, tfq = vq.twin(seg)
        try:
            want = oracle.execute(twin.data, tfq.spec)
            exp = F.expected(twin, tfq)
            F.check_result(twin, tfq, want, exp)
            mask = V.model_mask(seg, vq)
            assert np.array_equal(mask, exp.mask), "the user's part AND the valid mask is not the twin's filter"
            if tfq.tree is not None:
                words, card = oracle.filter_bitmap(twin.data, tfq.spec)
                assert card == int(mask.sum()) and np.array_equal(words, F.mask_words(mask)), "oracle.filter_bitmap differs from the model's mask"
            # the lists of the model
            m = V.model(seg, vq, mask)
            lists = m.lists if vq.group_by else {(): m.lists}
            if vq.group_by:
                assert sorted(lists, key=repr) == sorted(exp.groups, key=repr), "the value model's groups are not F.expected's"
            total = 0
            for key, per in lists.items():
                for a, (listed, docs) in per.items():
                    col = seg.cols[vq.aggs[a][1]]
                    total += len(docs) if a == vq.value_positions[0] else 0
                    if m.whole_dictionary:
                        assert len(listed) == col.cardinality
                        continue
                    if vq.family == Q.PERCENTILE:
                        assert int(listed[1].astype(np.int64).sum()) == len(docs)
                        values = RV.double_of_bits(listed[0], col.is_fp) if vq.raw else np.asarray(col.dict_values)[listed[0]].astype(np.float64)
                        expanded = np.repeat(values, listed[1].astype(np.int64))
                        for p in V.PERCENTILES:
                            a_p = V.model_percentile(col, docs, p)
                            b_p = float(expanded[V.P.percentile_index(len(expanded), p)]) if len(expanded) else float("-inf")
                            assert a_p == b_p or (np.isnan(a_p) and np.isnan(b_p)), (p, a_p, b_p)
                    else:
                        assert len(listed if not vq.raw else listed[0]) == len(np.unique(RV.order_image(col.values[docs])) if vq.raw else np.unique(col.ids[docs]))
            assert total == int(mask.sum())
        except AssertionError as e:
            raise AssertionError("%s: %s" % (where, e)) from e


# Coverage of the committed seed set (PINOT_FUZZ_SEED_BASE=0): what the seeds produce, measured; each label is held to half of its figure.
MEASURED = {
    "derived": 692, "dict_set_leaves:2+": 24, "doc_set:none": 501, "doc_set:roaring": 88, "doc_set:words": 103, "doc_set_density:empty": 45,
    "doc_set_density:full": 44, "doc_set_density:partial": 102, "encoding:DISTINCTCOUNT:dict_double": 71, "encoding:DISTINCTCOUNT:dict_float": 69,
    "encoding:DISTINCTCOUNT:dict_int": 240, "encoding:DISTINCTCOUNT:dict_long": 38, "encoding:DISTINCTCOUNT:raw_double": 82,
    "encoding:DISTINCTCOUNT:raw_float": 64, "encoding:DISTINCTCOUNT:raw_int": 96, "encoding:DISTINCTCOUNT:raw_long": 106,
    "encoding:PERCENTILE:dict_double": 75, "encoding:PERCENTILE:dict_float": 75, "encoding:PERCENTILE:dict_int": 236, "encoding:PERCENTILE:dict_long": 49,
    "encoding:PERCENTILE:raw_double": 86, "encoding:PERCENTILE:raw_float": 82, "encoding:PERCENTILE:raw_int": 97, "encoding:PERCENTILE:raw_long": 85,
    "encoding:dict_double": 146, "encoding:dict_float": 144, "encoding:dict_int": 476, "encoding:dict_long": 87, "encoding:raw_double": 168,
    "encoding:raw_float": 146, "encoding:raw_int": 193, "encoding:raw_long": 191, "extras": 260, "function:DISTINCTCOUNT": 346, "function:PERCENTILE":
    346, "grouped:DISTINCTCOUNT": 139, "grouped:PERCENTILE": 139, "grouped:no": 414, "grouped:yes": 278, "inverted_leaf": 60,
    "is_null_under_null_handling": 8, "key_scale:dict": 282, "key_scale:offset": 14, "keys:0": 414, "keys:1": 260, "keys:2": 18, "leaf:dict_range": 234,
    "leaf:dict_set": 192, "leaf:doc_range": 66, "leaf:inverted_range": 38, "leaf:inverted_set": 30, "leaf:is_null": 40, "leaf:match_all": 44,
    "leaf:match_none": 44, "leaf:raw_range": 124, "leaf:raw_set": 136, "leaf:raw_set_f64": 98, "leaves:0": 110, "leaves:1": 366, "leaves:2": 74,
    "leaves:3+": 142, "null_handling:off": 552, "null_handling:on": 140, "pass_alone:DISTINCTCOUNT:dict": 66, "pass_alone:DISTINCTCOUNT:raw": 79,
    "pass_alone:PERCENTILE:dict": 59, "pass_alone:PERCENTILE:raw": 63, "pass_alone:no": 425, "pass_alone:yes": 267, "shared_pred": 46, "value_columns:1":
    196, "value_columns:2": 241, "value_columns:3": 147, "value_columns:4": 108, "value_has:inf": 171, "value_has:nan": 109, "value_has:zero": 370,
    "variant:base": 496, "variant:small-key": 196, "whole_dictionary": 9,
}
COVERAGE_THRESHOLDS = {label: max(1, figure // 2) for label, figure in MEASURED.items()}


def test_the_derivation_covers_what_it_is_meant_to():
    if F.SEED_BASE != 0:
        return                  # a soak over other seeds: the thresholds are those of the committed seed set
    c = V.coverage((generated(seed)[0], generated(seed)[2]) for seed in F.SEEDS)
    short = {k: (c[k], need) for k, need in COVERAGE_THRESHOLDS.items() if c[k] < need}
    assert not short, "the derivation narrowed: %r" % short
    assert len(COVERAGE_THRESHOLDS) >= 50
    assert c["grouped:yes"] >= 40 and c["grouped:DISTINCTCOUNT"] >= 20 and c["grouped:PERCENTILE"] >= 20
