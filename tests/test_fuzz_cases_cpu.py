"""CPU tier of the typed fuzz (tests/fuzz_cases.py): for every seed tests/test_gpu_fuzz_typed.py uses, the oracle answers EVERY generated
query and agrees with the exact model -- filter bitmaps bit for bit, docs scanned, groups by key value, counts, integer sums exactly,
MIN / MAX by both of the reference's rules (aggregation-only Math.min / Math.max: NaN wins; group-by `value < holder`: NaN ignored),
FLOAT / DOUBLE sums within count * 2^-53 * sum|x| of math.fsum (the oracle's doc order is one order of the additions the bound covers), NaN
and infinite sums as such.  A reference side that declines nothing is what keeps the GPU test's decline cap honest.  The last test holds the
generator itself to what it is meant to cover, so that it cannot narrow unnoticed."""
import numpy as np
import pytest

import fuzz_cases as F
from oracle import oracle

_CACHE = {}


def generated(seed):
    if seed not in _CACHE:
        seg = F.make_segment(seed)
        _CACHE[seed] = (seg, F.make_queries(seg))
    return _CACHE[seed]


@pytest.mark.parametrize("seed", F.SEEDS)
def test_oracle_answers_every_generated_query_like_the_exact_model(seed):
    seg, queries = generated(seed)
    assert len(queries) == F.QUERIES_PER_SEGMENT
    for qi, fq in enumerate(queries):
        got = oracle.execute(seg.data, fq.spec)            # raises on a decline: there is none
        exp = F.expected(seg, fq)
        try:
            F.check_result(seg, fq, got, exp)
            if fq.tree is not None:
                words, card = oracle.filter_bitmap(seg.data, fq.spec)
                assert card == int(exp.mask.sum()) and np.array_equal(words, F.mask_words(exp.mask))
        except AssertionError as e:
            raise AssertionError("seed %d query %d (n=%d, aggs=%r, group_by=%r, null_handling=%r, limit=%d, leaves=%r): %s" % (
                seed, qi, seg.n, [(f, seg.cols[c].kind if c >= 0 else "*") for f, c in fq.aggs], [seg.cols[g].kind for g in fq.group_by],
                fq.null_handling, fq.limit, [x.kind for x in fq.leaves()], e)) from e


# Coverage of the committed seed set (PINOT_FUZZ_SEED_BASE=0), each label at least this often: about half of what the seeds produce.
COVERAGE_THRESHOLDS = {
    "aggregated_column:dict_double": 29, "aggregated_column:dict_float": 29, "aggregated_column:dict_int": 103, "aggregated_column:dict_long": 16,
    "aggregated_column:raw_double": 24, "aggregated_column:raw_float": 20, "aggregated_column:raw_int": 49, "aggregated_column:raw_long": 24,
    "aggregated_has:inf": 27, "aggregated_has:nan": 27, "aggregated_has:zero": 65, "filter_column:dict_double": 17, "filter_column:dict_float": 9,
    "filter_column:dict_int": 70, "filter_column:dict_long": 5, "filter_column:raw_double": 16, "filter_column:raw_float": 23,
    "filter_column:raw_int": 37, "filter_column:raw_long": 23, "function:avg": 74, "function:count": 91, "function:max": 74, "function:min": 84,
    "function:sum": 63, "group_by:0": 101, "group_by:1": 23, "group_by:2": 19, "group_min_max_has:inf": 8, "group_min_max_has:nan": 10,
    "group_min_max_has:zero": 18, "key_column:dict_double": 9, "key_column:dict_float": 4, "key_column:dict_int": 20, "key_column:dict_long": 7,
    "key_column:raw_double": 2, "key_column:raw_float": 6, "key_column:raw_int": 9, "key_column:raw_long": 2, "key_has:inf": 5, "key_has:nan": 6,
    "key_has:zero": 10, "key_scale:dict": 42, "key_scale:offset": 6, "key_scale:rank": 14, "leaf:dict_range": 45, "leaf:dict_set": 35,
    "leaf:doc_range": 17, "leaf:inverted_range": 10, "leaf:inverted_set": 10, "leaf:is_null": 10, "leaf:match_all": 13, "leaf:match_none": 10,
    "leaf:raw_range": 31, "leaf:raw_range_f64": 16, "leaf:raw_set": 29, "leaf:raw_set_f64": 23, "limit_set": 24, "min_max_dict_fp_nan": 8,
    "null_handling:off": 112, "null_handling:on": 32, "range_lo_above_hi": 7, "set_exclusive": 12, "set_size:1": 12, "set_size:cap": 8,
    "shared_pred": 12, "size:1": 1, "size:140000": 1, "size:20011": 1, "size:2047": 1, "size:2048": 1, "size:2049": 1, "size:4097": 1, "size:63": 1,
    "size:64": 1, "size:65": 1, "size:70001": 1, "sum_pool:benign": 11, "sum_pool:ill": 18, "sum_pool:special": 17,
}


def test_the_generator_covers_what_it_is_meant_to():
    if F.SEED_BASE != 0:
        return                  # a soak over other seeds: the thresholds are those of the committed seed set
    c = F.coverage(generated(seed) for seed in F.SEEDS)
    short = {k: (c[k], need) for k, need in COVERAGE_THRESHOLDS.items() if c[k] < need}
    assert not short, "the generator narrowed: %r" % short
    assert len(COVERAGE_THRESHOLDS) >= 60
