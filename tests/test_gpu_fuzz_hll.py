"""Randomised parity of DISTINCTCOUNTHLL behind general filter trees (tests/fuzz_hll_cases.py): scan_hll_kernel / group_hll_kernel on raw columns,
scan_distinct_kernel / group_distinct_kernel + hll_fold_kernel on dictionary columns -- re-evaluating the lowered filter with
eval_filter_private, reading index_and_kernel's tile list, sharing the per-query scratch with a DISTINCTCOUNT's bitsets -- against an exact
model, the ordinary query beside them against the oracle and the typed fuzz's model.  PINOT_GPU_COLLECT stays unset: raw HLL has no switch.

Per derived query, through the C ABI:
  * the registers against the model byte for byte, per group by key value (hll_cases.assert_one_register_set: count = the non-zero
    registers, sum 0, min +inf, max -inf); a DISTINCTCOUNT beside the HLLs against its set (fuzz_value_cases.check_value); two aggregations
    of one (column, log2m) hold identical bytes;
  * the ordinary aggregations, the group set and the statistics against F.expected of the companion query (HLL and DISTINCTCOUNT turned
    into COUNT(*)) and against the oracle on the same companion (helpers.assert_results_equal, check_stats=True); numEntriesScannedPostFilter
    is numDocsScanned x the distinct columns of the ORIGINAL query, 0 when the dictionaries answered; numEntriesScannedInFilter equals the
    oracle's whenever both flag it exact;
  * pg_filter_bitmap bit for bit against the model's mask (queries without GROUP BY);
  * every executed query of the segment once more through ONE pg_execute_batch, twice, with its companion query as an item beside it: both
    calls are checked like the single execution and hold registers, sets and ordinary fields identical to its own (but FLOAT / DOUBLE
    sums, which the device adds in no fixed order: the model's bound holds those); companion items: F.check_result, both calls;
  * declines: PG_ERR_UNSUPPORTED only, with a message of fuzz_cases.DECLINE_ALLOW_LIST or one of the two size messages the DATA decides
    (fuzz_hll_cases.SIZE_DECLINES), at most MAX_DECLINED of the derived queries.  tests/test_fuzz_hll_cases_cpu.py shows the reference side
    declines nothing and that the size messages reach 1 of the 341 derived queries of the committed seeds.
Each case must reach scan_hll_kernel and scan_distinct_kernel from queries that are the pass alone, two segments each (index_and_kernel may
outlast the pass of an index-driven filter: those are not counted), and execute at least MIN_GROUPED grouped queries.  The fuzz's
dictionaries are small: only PINOT_GPU_DISTINCT_LDS=0 reaches the bitsets' HBM tier, which the fold must read as it reads the LDS tier's.

Measured on an MI355X (the committed seeds; the test_gpu_fuzz_values.py cases took 1.9 - 18.0 s in the same run), the same for all four
(grid, bitset tier) settings of a seed half:
  even seeds: 171 derived, 168 executed (65 grouped, 51 the pass alone, 0 of 42 without an exact entry count), 3 declined,
              pass kernels reached from {scan_distinct_kernel: 12, scan_hll_kernel: 11} segments, 1.1 - 1.3 s per case;
  odd seeds:  170 derived, 166 executed (65 grouped, 50 the pass alone, 0 of 36 without an exact entry count), 4 declined,
              pass kernels reached from {scan_distinct_kernel: 11, scan_hll_kernel: 11} segments, 2.2 - 2.4 s per case."""
import re
import time

import numpy as np
import pytest

import fuzz_cases as F
import fuzz_hll_cases as FH
import fuzz_value_cases as V
import helpers as H
from oracle import oracle
from pinot_amd import _abi
from pinot_amd import query as Q
from test_gpu_doc_set import MAX_STATS_LEFT_OUT
from test_gpu_fuzz_typed import MAX_DECLINED
from test_gpu_fuzz_values import MIN_GROUPED, Tally, create_doc_set

pytestmark = pytest.mark.gpu

REQUIRED_PASS_KERNELS = ["scan_hll_kernel", "scan_distinct_kernel"]


def check_query(seg, hq, got, twin, tfq, want, exp, m):
    FH.check_values(seg, hq, got, m)
    view = V.ordinary_view(hq, got, want, seg, m)
    F.check_result(twin, tfq, view, exp)
    # FLOAT / DOUBLE sums over ill-conditioned columns have been held to the model's bound above; the helper's tolerance means nothing there
    for i, (f, c) in enumerate(tfq.aggs):
        if f in (Q.SUM, Q.AVG) and c >= 0 and twin.cols[c].pool == "ill":
            rows = [(view.aggregations, want.aggregations)] if not hq.group_by else [(view.groups[k], want.groups[k]) for k in view.groups if k in want.groups]
            for mine, theirs in rows:
                if mine:
                    mine[i].sum = theirs[i].sum
    H.assert_results_equal(view, want, check_stats=True)
    assert got.group_keys == want.group_keys and got.num_groups_limit_reached == want.num_groups_limit_reached
    if m.whole_dictionary:
        assert got.stats == (seg.n, 0, 0, seg.n), "the dictionaries answer: statistics %r" % (got.stats,)
    if hq.counts_only and not hq.group_by and not m.whole_dictionary:
        counts = [got.aggregations[a].count for a, (f, c) in enumerate(hq.aggs) if f == Q.COUNT]
        assert all(n == got.stats[0] for n in counts), "the pass alone: counts %r, numDocsScanned %d" % (counts, got.stats[0])


def run_seed_set(engine, seeds, tally):
    for seed in seeds:
        seg = F.make_segment(seed)
        hqs = FH.make_hll_queries(seg, F.make_queries(seg))
        tally.derived += len(hqs)
        ran, doc_sets = [], {}
        with engine.open(seg.data) as g:
            for hq in hqs:
                where = "seed %d %s" % (seed, hq.describe(seg))
                doc_set = doc_sets[id(hq)] = create_doc_set(g, hq)
                spec = hq.device(doc_set).spec
                try:
                    got = g.execute(spec)
                except _abi.PinotGpuError as e:
                    assert e.status == _abi.PG_ERR_UNSUPPORTED, "%s: %s" % (where, e)
                    assert any(re.search(p, str(e)) for p in F.DECLINE_ALLOW_LIST + FH.SIZE_DECLINES), "%s: declined outside the allow-list: %s" % (where, e)
                    tally.declined += 1
                    tally.reasons.append(re.sub(r"\d+", "N", str(e))[:90])
                    continue
                twin, tfq = hq.twin(seg)
                want = oracle.execute(twin.data, tfq.spec)
                exp = F.expected(twin, tfq)
                m = FH.model(seg, hq)
                try:
                    assert np.array_equal(m.mask, exp.mask), "the model's mask is not the twin's"
                    check_query(seg, hq, got, twin, tfq, want, exp, m)
                    pass_alone = hq.counts_only and not hq.group_by and not m.whole_dictionary
                    if pass_alone:
                        tally.pass_alone += 1
                        if want.filter_entries_exact:
                            tally.pass_alone_exact_wanted += 1
                            tally.left_out += not got.filter_entries_exact
                        if got.dominant_kernel_ms > 0.0:          # (0.0: nothing was launched)
                            # the pass's kernel, or index_and_kernel outlasting it; a raw column never reports the dictionary pass and vice versa
                            assert got.dominant_kernel != ("scan_distinct_kernel" if hq.raw else "scan_hll_kernel"), "the pass alone reports %s" % got.dominant_kernel
                            tally.reached.setdefault(got.dominant_kernel, set()).add(seed)
                    if not hq.group_by:
                        words, card = g.filter_bitmap(hq.device(doc_set, companion=True).spec)
                        assert card == int(m.mask.sum()) and np.array_equal(words, F.mask_words(m.mask)), "filter bitmap"
                except AssertionError as e:
                    raise AssertionError("%s [%s]: %s" % (where, got.dominant_kernel, e)) from e
                tally.executed += 1
                tally.grouped += bool(hq.group_by)
                ran.append((hq, spec, got, twin, tfq, want, exp, m))
            # the segment's queries and their companions in ONE pg_execute_batch, twice
            companions = [hq.device(doc_sets[id(hq)], companion=True).spec for hq, *_ in ran]
            for rep in range(2):
                out = engine.execute_batch([g] * (2 * len(ran)), [r[1] for r in ran] + companions) if ran else []
                for k, ((status, res), (hq, spec, single, twin, tfq, want, exp, m)) in enumerate(zip(out, ran + ran)):
                    assert status == _abi.PG_OK, "seed %d: batch status %d (%s)" % (seed, status, hq.describe(seg))
                    try:
                        if k >= len(ran):
                            F.check_result(twin, tfq, res, exp)
                            continue
                        FH.same_results(res, single, hq)
                        check_query(seg, hq, res, twin, tfq, want, exp, m)
                    except AssertionError as e:
                        raise AssertionError("seed %d batch pass %d item %d %s: %s" % (seed, rep, k, hq.describe(seg), e)) from e


@pytest.mark.parametrize("tier", [None, "0"], ids=["tiers-by-size", "hbm-tier"])
@pytest.mark.parametrize("cus", [None, "1"], ids=["whole-device", "one-cu"])
@pytest.mark.parametrize("half", [0, 1], ids=["even-seeds", "odd-seeds"])
def test_random_hll_queries_behind_general_filters(engine, half, cus, tier):
    seeds = F.SEEDS[half::2]          # (the seed set in two halves, each with every segment size)
    engine.reinit(PINOT_GPU_TEST_CUS=cus, PINOT_GPU_DISTINCT_LDS=tier)
    tally = Tally()
    tally.reasons = []
    started = time.perf_counter()
    try:
        run_seed_set(engine, seeds, tally)
    finally:
        engine.reinit(PINOT_GPU_TEST_CUS=None, PINOT_GPU_DISTINCT_LDS=None)
    print("value fuzz DISTINCTCOUNTHLL: %d derived, %d executed (%d grouped, %d the pass alone of which %d of %d without an exact entry count), %d declined, kernels %r, %.1f s" % (
        tally.derived, tally.executed, tally.grouped, tally.pass_alone, tally.left_out, tally.pass_alone_exact_wanted, tally.declined,
        {k: len(v) for k, v in sorted(tally.reached.items())}, time.perf_counter() - started))
    print("declined: %r" % sorted(tally.reasons))
    assert tally.executed + tally.declined == tally.derived
    assert tally.declined <= MAX_DECLINED * tally.derived, "%d of %d derived queries declined" % (tally.declined, tally.derived)
    assert tally.left_out <= MAX_STATS_LEFT_OUT * tally.pass_alone_exact_wanted, "%d of %d pass-alone queries without an exact entry count" % (tally.left_out, tally.pass_alone_exact_wanted)
    missing = {k: sorted(tally.reached.get(k, ())) for k in REQUIRED_PASS_KERNELS if len(tally.reached.get(k, ())) < 2}
    assert not missing, "pass kernels reached from fewer than two segments: %r (reached: %r)" % (missing, {k: len(v) for k, v in tally.reached.items()})
    assert tally.grouped >= MIN_GROUPED, "%d grouped queries executed" % tally.grouped
