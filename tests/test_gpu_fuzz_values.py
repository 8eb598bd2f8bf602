"""Randomised parity of DISTINCTCOUNT / PERCENTILE behind general filter trees (tests/fuzz_value_cases.py): the value passes -- bitsets, counter
vectors, collected and sorted lists, re-evaluating the lowered filter with eval_filter_private -- against an exact model, the ordinary query
beside them against the oracle and the typed fuzz's model.  Runs under PINOT_GPU_COLLECT=1 (the raw columns' collect pass).

Per derived query, through the C ABI:
  * the sets, lists and counts against the model, element for element, per group by key value; PERCENTILE's final answers for
    p = 0, 50, 90, 99, 100 from the returned runs against a sort of the matching docs' doubles (== or both NaN);
  * the ordinary aggregations, the group set and the statistics against F.expected of the companion query (value functions turned into
    COUNT(*)) and against the oracle on the same companion (helpers.assert_results_equal, check_stats=True); numEntriesScannedPostFilter is
    numDocsScanned x the distinct columns of the ORIGINAL query; numEntriesScannedInFilter equals the oracle's whenever both flag it exact;
  * a query of value functions and COUNT(*) without GROUP BY (the pass alone, which produces the statistics itself): count of every
    PERCENTILE == numDocsScanned == COUNT(*); at most test_gpu_doc_set.MAX_STATS_LEFT_OUT of those the oracle counts exactly may come back
    without an exact entry count;
  * pg_filter_bitmap bit for bit against the model's mask (queries without GROUP BY);
  * every executed query of the segment once more through ONE pg_execute_batch, twice, with its companion query (value functions turned
    into COUNT(*)) as an item beside it.  A value item runs as a pg_execute of its own on the library's worker threads, side by side with
    the others, and never enters the plan cache: its second call is a repeat; the companion items are what the second call finds in the
    plan cache.  Value items: both calls are checked like the single execution and hold lists and ordinary fields identical to
    its own (but FLOAT / DOUBLE sums, which the device adds in no fixed order: the model's bound holds those);
    companion items: F.check_result against the model, both calls;
  * declines: PG_ERR_UNSUPPORTED only, with a message of fuzz_cases.DECLINE_ALLOW_LIST or of PRICING_DECLINES below, at most 10 % of the
    derived queries.  The derivation removes every decline that the query's SHAPE decides (tests/test_fuzz_value_cases_cpu.py holds it to
    that and shows the reference side declines nothing).  PRICING_DECLINES adds the three declines that the DATA decides -- the size of what
    the pass would allocate, known only from the cardinalities and the doc count:
      "DISTINCTCOUNT bit matrices of %llu bytes exceed ..."      (PG_DISTINCT_GROUP_MAX_BYTES / the PINOT_GPU_GROUP_TABLE_BYTES budget)
      "PERCENTILE counter matrices of %llu bytes exceed ..."     (PG_PERCENTILE_GROUP_MAX_BYTES / the budget)
      "... value lists of %llu bytes over raw columns exceed ..." (PG_COLLECT_MAX_BYTES / the budget)
Each family's run must reach its pass kernels from queries that are the pass alone (REQUIRED_PASS_KERNELS, two segments each;
index_and_kernel may outlast the pass of an index-driven filter: those are not counted) and execute at least MIN_GROUPED grouped queries.
The fuzz's dictionaries are small: only the tier switch (PINOT_GPU_DISTINCT_LDS=0 / PINOT_GPU_PERCENTILE_LDS=0) reaches the HBM tiers."""
import re
import time

import numpy as np
import pytest

import fuzz_cases as F
import fuzz_value_cases as V
import helpers as H
from oracle import oracle
from pinot_amd import _abi
from pinot_amd import query as Q
from test_gpu_doc_set import MAX_STATS_LEFT_OUT
from test_gpu_fuzz_typed import MAX_DECLINED

pytestmark = pytest.mark.gpu

PRICING_DECLINES = [
    r"DISTINCTCOUNT bit matrices of \d+ bytes exceed",
    r"PERCENTILE counter matrices of \d+ bytes exceed",
    r"value lists of \d+ bytes over raw columns exceed",
]
REQUIRED_PASS_KERNELS = {Q.DISTINCTCOUNT: ["scan_distinct_kernel", "scan_collect_kernel"], Q.PERCENTILE: ["scan_counts_kernel", "scan_collect_kernel"]}
TIER_SWITCH = {Q.DISTINCTCOUNT: "PINOT_GPU_DISTINCT_LDS", Q.PERCENTILE: "PINOT_GPU_PERCENTILE_LDS"}
MIN_GROUPED = 20


def create_doc_set(g, vq):
    if vq.valid is None:
        return None
    if vq.valid_format == "roaring":
        return g.create_doc_set(doc_ids=np.flatnonzero(vq.valid).astype(np.int32))
    return g.create_doc_set(words=F.mask_words(vq.valid))


def check_query(seg, vq, got, twin, tfq, want, exp, m):
    V.check_values(seg, vq, got, m)
    view = V.ordinary_view(vq, got, want, seg, m)
    F.check_result(twin, tfq, view, exp)
    # FLOAT / DOUBLE sums over ill-conditioned columns have been held to the model's bound above; the helper's tolerance means nothing there
    for i, (f, c) in enumerate(tfq.aggs):
        if f in (Q.SUM, Q.AVG) and c >= 0 and twin.cols[c].pool == "ill":
            rows = [(view.aggregations, want.aggregations)] if not vq.group_by else [(view.groups[k], want.groups[k]) for k in view.groups if k in want.groups]
            for mine, theirs in rows:
                if mine:
                    mine[i].sum = theirs[i].sum
    H.assert_results_equal(view, want, check_stats=True)
    assert got.group_keys == want.group_keys and got.num_groups_limit_reached == want.num_groups_limit_reached
    if vq.counts_only and not vq.group_by and not m.whole_dictionary:
        counts = [got.aggregations[a].count for a, (f, c) in enumerate(vq.aggs) if f == Q.PERCENTILE or f == Q.COUNT]
        assert all(n == got.stats[0] for n in counts), "the pass alone: counts %r, numDocsScanned %d" % (counts, got.stats[0])


class Tally:
    def __init__(self):
        self.derived = self.executed = self.declined = self.grouped = self.pass_alone = self.pass_alone_exact_wanted = self.left_out = 0
        self.reached = {}


def run_seed_set(engine, family, seeds, tally):
    for seed in seeds:
        seg = F.make_segment(seed)
        vqs = [v for v in V.make_value_queries(seg, F.make_queries(seg)) if v.family == family]
        tally.derived += len(vqs)
        ran, doc_sets = [], {}
        with engine.open(seg.data) as g:
            for vq in vqs:
                where = "seed %d %s" % (seed, vq.describe(seg))
                doc_set = doc_sets[id(vq)] = create_doc_set(g, vq)
                spec = vq.device(doc_set).spec
                try:
                    got = g.execute(spec)
                except _abi.PinotGpuError as e:
                    assert e.status == _abi.PG_ERR_UNSUPPORTED, "%s: %s" % (where, e)
                    assert any(re.search(p, str(e)) for p in F.DECLINE_ALLOW_LIST + PRICING_DECLINES), "%s: declined outside the allow-list: %s" % (where, e)
                    tally.declined += 1
                    continue
                twin, tfq = vq.twin(seg)
                want = oracle.execute(twin.data, tfq.spec)
                exp = F.expected(twin, tfq)
                m = V.model(seg, vq)
                try:
                    assert np.array_equal(m.mask, exp.mask), "the model's mask is not the twin's"
                    check_query(seg, vq, got, twin, tfq, want, exp, m)
                    pass_alone = vq.counts_only and not vq.group_by and not m.whole_dictionary
                    if pass_alone:
                        tally.pass_alone += 1
                        if want.filter_entries_exact:
                            tally.pass_alone_exact_wanted += 1
                            tally.left_out += not got.filter_entries_exact
                        if got.dominant_kernel_ms > 0.0:          # (0.0: nothing was launched)
                            # the pass's kernel, or index_and_kernel outlasting it; a raw column never reports a dictionary pass and vice versa
                            assert got.dominant_kernel != (REQUIRED_PASS_KERNELS[family][0] if vq.raw else "scan_collect_kernel"), "the pass alone reports %s" % got.dominant_kernel
                            tally.reached.setdefault(got.dominant_kernel, set()).add(seed)
                    if not vq.group_by:
                        words, card = g.filter_bitmap(vq.device(doc_set, companion=True).spec)
                        assert card == int(m.mask.sum()) and np.array_equal(words, F.mask_words(m.mask)), "filter bitmap"
                except AssertionError as e:
                    raise AssertionError("%s [%s]: %s" % (where, got.dominant_kernel, e)) from e
                tally.executed += 1
                tally.grouped += bool(vq.group_by)
                ran.append((vq, spec, got, twin, tfq, want, exp, m))
            # the segment's queries and their companions in ONE pg_execute_batch, twice
            companions = [vq.device(doc_sets[id(vq)], companion=True).spec for vq, *_ in ran]
            for rep in range(2):
                out = engine.execute_batch([g] * (2 * len(ran)), [r[1] for r in ran] + companions) if ran else []
                for k, ((status, res), (vq, spec, single, twin, tfq, want, exp, m)) in enumerate(zip(out, ran + ran)):
                    assert status == _abi.PG_OK, "seed %d: batch status %d (%s)" % (seed, status, vq.describe(seg))
                    try:
                        if k >= len(ran):
                            F.check_result(twin, tfq, res, exp)
                            continue
                        V.same_value_lists(res, single, vq)
                        check_query(seg, vq, res, twin, tfq, want, exp, m)
                    except AssertionError as e:
                        raise AssertionError("seed %d batch pass %d item %d %s: %s" % (seed, rep, k, vq.describe(seg), e)) from e


@pytest.mark.parametrize("tier", [None, "0"], ids=["tiers-by-size", "hbm-tier"])
@pytest.mark.parametrize("cus", [None, "1"], ids=["whole-device", "one-cu"])
@pytest.mark.parametrize("family", [Q.DISTINCTCOUNT, Q.PERCENTILE], ids=["DISTINCTCOUNT", "PERCENTILE"])
@pytest.mark.parametrize("half", [0, 1], ids=["even-seeds", "odd-seeds"])
def test_random_value_queries_behind_general_filters(engine, half, family, cus, tier):
    seeds = F.SEEDS[half::2]          # (the seed set in two halves, each with every segment size: a case stays within a few seconds)
    engine.reinit(**{"PINOT_GPU_COLLECT": "1", "PINOT_GPU_TEST_CUS": cus, TIER_SWITCH[family]: tier})
    tally = Tally()
    started = time.perf_counter()
    try:
        run_seed_set(engine, family, seeds, tally)
    finally:
        engine.reinit(**{"PINOT_GPU_COLLECT": None, "PINOT_GPU_TEST_CUS": None, TIER_SWITCH[family]: None})
    print("value fuzz %s: %d derived, %d executed (%d grouped, %d the pass alone of which %d of %d without an exact entry count), %d declined, kernels %r, %.1f s" % (
        V.FAMILIES[family], tally.derived, tally.executed, tally.grouped, tally.pass_alone, tally.left_out, tally.pass_alone_exact_wanted, tally.declined,
        {k: len(v) for k, v in sorted(tally.reached.items())}, time.perf_counter() - started))
    assert tally.executed + tally.declined == tally.derived
    assert tally.declined <= MAX_DECLINED * tally.derived, "%d of %d derived queries declined" % (tally.declined, tally.derived)
    assert tally.left_out <= MAX_STATS_LEFT_OUT * tally.pass_alone_exact_wanted, "%d of %d pass-alone queries without an exact entry count" % (tally.left_out, tally.pass_alone_exact_wanted)
    missing = {k: sorted(tally.reached.get(k, ())) for k in REQUIRED_PASS_KERNELS[family] if len(tally.reached.get(k, ())) < 2}
    assert not missing, "pass kernels reached from fewer than two segments: %r (reached: %r)" % (missing, {k: len(v) for k, v in tally.reached.items()})
    assert tally.grouped >= MIN_GROUPED, "%d grouped queries executed" % tally.grouped
