"""CPU tier of the wide-key group-by fuzz (tests/fuzz_group_cases.py): for every seed tests/test_gpu_fuzz_groups.py uses, the oracle answers
EVERY generated query and agrees with the exact model of tests/fuzz_cases.py -- docs scanned, groups by key value, counts, integer sums
exactly, MIN / MAX, DOUBLE sums within count * 2^-53 * sum|x| -- and its rows carry the raw keys the generator computes from the key
digits (under a binding numGroupsLimit: the first keys in docId order, group_map_cases.admitted_keys).  The other tests hold the generator
to what it exists for: every record format and plan class of the partitioned path from at least two segments, every key distribution,
every fixed filter kind, every limit kind, and no query that a documented decline rule would catch."""
import numpy as np
import pytest

import fuzz_cases as F
import fuzz_group_cases as G
import group_map_cases as GM
from oracle import oracle

_CACHE = {}


def generated(seed):
    if seed not in _CACHE:
        seg = G.make_segment(seed)
        _CACHE[seed] = (seg, G.make_queries(seg))
    return _CACHE[seed]


def expected_raw_keys(seg, fq, exp):
    """The raw keys of the rows the model expects: every key of the matching docs, or the first min(product, limit) in docId order when
    the holder is map based (fuzz_cases.expected states when it is)."""
    raw = G.raw_keys(seg, fq)
    present = set(int(k) for k in np.unique(raw[exp.mask]))
    if len(exp.groups) == len(present):
        return present
    return GM.admitted_keys(raw, exp.mask, len(exp.groups))


def where(seg, qi, fq):
    info = fq.info
    return "seed %d query %d [%s / %s, n=%d, target %s, %s, product %d, shift %d, 2^%d per coarse, %d accumulators, packed %d, filter %s, limit %d (%s), null_handling %r]" % (
        seg.seed, qi, fq.shape, info.klass, seg.n, seg.target, seg.distribution, info.product, info.shift, info.log2_fine_per_coarse, len(info.accumulators),
        info.packed_bits, fq.filter_kind, fq.limit, fq.limit_kind, fq.null_handling)


@pytest.mark.parametrize("seed", G.SEEDS)
def test_oracle_answers_every_generated_query_like_the_exact_model(seed):
    seg, queries = generated(seed)
    assert len(queries) == len(G.QUERY_SHAPES)
    for qi, fq in enumerate(queries):
        got = oracle.execute(seg.data, fq.spec)            # raises on a decline: there is none
        exp = F.expected(seg, fq)
        try:
            F.check_result(seg, fq, got, exp)
            assert set(got.groups) == expected_raw_keys(seg, fq, exp), "raw keys of the rows"
            assert list(got.groups) == sorted(got.groups)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (where(seg, qi, fq), e)) from e


def test_the_planner_arithmetic_at_its_boundaries():
    """G.plan against the figures the issue's boundary cases are named for (pg_engine.hip:4672-4685)."""
    assert G.plan(1 << 21, 2) == (12, 512, 0, 512) and G.plan((1 << 21) + 1, 2) == (12, 513, 1, 257)
    assert G.plan(1 << 20, 3) == (11, 512, 0, 512) and G.plan((1 << 20) + 1, 3) == (11, 513, 1, 257)
    assert G.plan(1 << 21, 3)[2] == 1 and G.plan(10_001, 0) == (12, 3, 0, 3)
    assert [G.plan(p, 1)[2] for p in (3_000_000, 6_000_000, 9_000_000)] == [1, 2, 3]
    assert G.plan(4099 * 4099 * 2, 1)[2] == 5 and G.plan(4099 * 4099 * 2, 3)[2] == 6


REQUIRED_CLASSES = ["one-level packed (COUNT only)", "one-level packed (one unsigned input)", "one-level unpacked, 1 accumulators",
                    "one-level unpacked, 2 accumulators", "one-level unpacked, 3 accumulators", "two-level packed", "two-level unpacked",
                    "fine per coarse 2^1", "fine per coarse 2^2", "fine per coarse 2^3", "wide", "more than 3 accumulators", "non-INT32 input", "lds"]


def test_the_seed_set_reaches_every_class_from_two_segments():
    if G.SEED_BASE != 0:
        return                  # a soak over other seeds: the requirement is on the committed seed set
    reached = {}
    for seed in G.SEEDS:
        seg, queries = generated(seed)
        reached.setdefault("distribution " + seg.distribution, set()).add(seed)
        reached.setdefault("size %d" % seg.n, set()).add(seed)
        for fq in queries:
            for label in fq.info.labels():
                reached.setdefault(label, set()).add(seed)
            if fq.info.partitionable:
                reached.setdefault("filter " + fq.filter_kind, set()).add(seed)
                reached.setdefault("limit " + fq.limit_kind, set()).add(seed)
                for g in fq.group_by:
                    reached.setdefault("key " + seg.cols[g].kind + (" forced width" if seg.cols[g].is_dict and seg.cols[g].column.bits > max(1, int(seg.cols[g].cardinality - 1).bit_length()) else ""), set()).add(seed)
                for _, c in fq.aggs:
                    if c >= 0:
                        reached.setdefault("input " + [r for r, i in seg.roles.items() if i == c][0], set()).add(seed)
                reached.setdefault("null handling %s" % fq.null_handling, set()).add(seed)
    need = REQUIRED_CLASSES + ["distribution " + d for d in G.DISTRIBUTIONS] + ["filter " + k for k in G.FIXED_FILTERS + ["tree", "none"]] + \
        ["limit " + k for k in ("0", "5", "200", "present", "present-1")] + ["size %d" % n for n in G.SIZES] + \
        ["key " + k for k in ("dict_int", "dict_int forced width", "dict_long", "dict_float", "dict_double", "raw_int")] + \
        ["input " + r for r in ("affine", "irregular", "edges", "long", "benign", "ill", "raw")] + ["null handling True", "null handling False"]
    short = {k: sorted(reached.get(k, ())) for k in need if len(reached.get(k, ())) < 2}
    assert not short, "reached from fewer than two segments: %r" % short


def test_lds_controls_are_not_map_based_and_wide_multipliers_pass_two_to_the_24():
    for seed in G.SEEDS:
        seg, queries = generated(seed)
        for fq in queries:
            if fq.shape == "lds":
                assert fq.info.klass == "lds" and not fq.info.map_based and not fq.info.partitionable
        if seg.target == "wide":
            cards = [seg.cols[k].key_scale()[2] for k in seg.keys]
            assert len(cards) == 3 and cards[0] * cards[1] > 1 << 24 and int(np.prod(cards)) <= 34_000_000
        if seg.n >= 2:
            raw = G.raw_keys(seg, queries[0])
            assert raw.min() == 0 and raw.max() == queries[0].info.product - 1 or queries[0].null_handling
    assert sum(G.TARGETS[s % len(G.TARGETS)] == "wide" for s in G.SEEDS) <= 2


def test_no_generated_query_matches_a_documented_decline():
    for seed in G.SEEDS:
        seg, queries = generated(seed)
        for qi, fq in enumerate(queries):
            assert G.static_decline(seg, fq) is None, "%s: %s" % (where(seg, qi, fq), G.static_decline(seg, fq))
