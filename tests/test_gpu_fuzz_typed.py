"""Randomised parity over raw and typed columns (tests/fuzz_cases.py): the device against the oracle AND against the exact model.

Per generated query, through the C ABI:
  * helpers.assert_results_equal(device, oracle, check_stats=True): numDocsScanned, numEntriesScannedPostFilter, total docs always,
    numEntriesScannedInFilter whenever both sides flag it exact;
  * the exact model: counts, groups by key value, integer sums exactly, MIN / MAX with NaN by isnan and everything else by == -- in a
    group the sign of a zero extreme is the first zero's in doc order in the reference and is not compared; aggregation-only
    Math.min / Math.max order the zeros and the sign is compared -- and FLOAT / DOUBLE sums: NaN / +inf / -inf exactly as the model's, finite
    ones within |device - math.fsum| <= count * 2^-53 * sum|x| (fuzz_cases.fp_sum_bound: any order of the additions stays inside; a
    float32 accumulation, a dropped tile or a double-counted tail does not).  On ill-conditioned columns that bound REPLACES the
    helper's tolerance, which assumes |value| <= 1e6 and a sum that does not cancel: the helper then sees the oracle's figure;
  * pg_filter_bitmap bit for bit against the model's mask (filters without group-by);
  * every query of the segment once more through pg_execute_batch, twice (the second call meets the plan cache): the same results
    and statistics as the single executions;
  * declines: PG_ERR_UNSUPPORTED only, with a message of fuzz_cases.DECLINE_ALLOW_LIST; at most 10 % of the seed set's queries.
The seed set must reach the kernels of REQUIRED_KERNELS, each from two segments, and runs twice: on the whole device and with
PINOT_GPU_TEST_CUS=1 (more tiles than waves)."""
import re

import numpy as np
import pytest

import fuzz_cases as F
import helpers as H
from device_results import same_results
from oracle import oracle
from pinot_amd import _abi
from pinot_amd import query as Q

pytestmark = pytest.mark.gpu

# dominant_kernel names (_abi.KERNEL_NAMES) the seed set has to reach, each from at least two different segments
REQUIRED_KERNELS = ["scan_raw_set_kernel", "scan_raw_kernel", "scan_simple_kernel", "scan_narrow_kernel", "scan_hist_kernel", "scan_private_kernel",
                    "scan_private_typed_kernel", "group_private_kernel", "scan_group_kernel"]
MAX_DECLINED = 0.10


def check_query(seg, fq, got, want, exp):
    F.check_result(seg, fq, got, exp)
    # FLOAT / DOUBLE sums over ill-conditioned columns have been held to the model's bound above; the helper's tolerance means nothing there
    for i, (f, c) in enumerate(fq.aggs):
        if f in (Q.SUM, Q.AVG) and c >= 0 and seg.cols[c].pool == "ill":
            for mine, theirs in [(got.aggregations, want.aggregations)] + [(got.groups[g], want.groups[g]) for g in got.groups if g in want.groups]:
                if mine:
                    mine[i].sum = theirs[i].sum
    H.assert_results_equal(got, want, check_stats=True)
    assert got.group_keys == want.group_keys and got.num_groups_limit_reached == want.num_groups_limit_reached


def run_seed_set(engine):
    reached = {}
    generated = declined = 0
    for seed in F.SEEDS:
        seg = F.make_segment(seed)
        queries = F.make_queries(seg)
        generated += len(queries)
        ran = []
        with engine.open(seg.data) as g:
            for qi, fq in enumerate(queries):
                where = "seed %d query %d (n=%d, aggs=%r, group_by=%r, null_handling=%r, limit=%d, leaves=%r)" % (
                    seed, qi, seg.n, [(f, seg.cols[c].kind if c >= 0 else "*") for f, c in fq.aggs], [seg.cols[k].kind for k in fq.group_by],
                    fq.null_handling, fq.limit, [x.kind for x in fq.leaves()])
                try:
                    got = g.execute(fq.spec)
                except _abi.PinotGpuError as e:
                    assert e.status == _abi.PG_ERR_UNSUPPORTED, "%s: %s" % (where, e)
                    assert any(re.search(p, str(e)) for p in F.DECLINE_ALLOW_LIST), "%s: declined outside the allow-list: %s" % (where, e)
                    declined += 1
                    continue
                want = oracle.execute(seg.data, fq.spec)
                exp = F.expected(seg, fq)
                try:
                    check_query(seg, fq, got, want, exp)
                    if fq.tree is not None and not fq.group_by:
                        words, card = g.filter_bitmap(fq.spec)
                        assert card == int(exp.mask.sum()) and np.array_equal(words, F.mask_words(exp.mask)), "filter bitmap"
                except AssertionError as e:
                    raise AssertionError("%s [%s]: %s" % (where, got.dominant_kernel, e)) from e
                reached.setdefault(got.dominant_kernel, set()).add(seed)
                ran.append((fq, got, want, exp))
            # the segment's queries in ONE pg_execute_batch, twice
            for rep in range(2):
                out = engine.execute_batch([g] * len(ran), [r[0].spec for r in ran]) if ran else []
                for (status, res), (fq, single, want, exp) in zip(out, ran):
                    assert status == _abi.PG_OK, "seed %d: batch status %d" % (seed, status)
                    try:
                        check_query(seg, fq, res, want, exp)
                        same_results(res, single)
                    except AssertionError as e:
                        raise AssertionError("seed %d batch pass %d (aggs=%r, group_by=%r, null_handling=%r): %s" % (seed, rep, fq.aggs, fq.group_by, fq.null_handling, e)) from e
    return reached, generated, declined


@pytest.mark.parametrize("cus", [None, "1"], ids=["whole-device", "one-cu"])
def test_random_typed_segments_and_queries(engine, cus):
    engine.reinit(PINOT_GPU_TEST_CUS=cus)
    try:
        reached, generated, declined = run_seed_set(engine)
    finally:
        engine.reinit(PINOT_GPU_TEST_CUS=None)
    print("typed fuzz: %d queries, %d declined, kernels %r" % (generated, declined, {k: len(v) for k, v in sorted(reached.items())}))
    assert declined <= MAX_DECLINED * generated, "%d of %d generated queries declined" % (declined, generated)
    missing = {k: sorted(reached.get(k, ())) for k in REQUIRED_KERNELS if len(reached.get(k, ())) < 2}
    assert not missing, "kernels reached from fewer than two segments: %r (reached: %r)" % (missing, {k: len(v) for k, v in reached.items()})
