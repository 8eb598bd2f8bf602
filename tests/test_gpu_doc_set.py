"""Doc sets on the device (pg_doc_set_*, PG_PRED_DOC_SET: the queryable docIds of an upsert / dedup segment), through the C ABI.
Expected values: the unchanged oracle over the TWIN segment of tests/doc_set_cases.py (tests/test_doc_set_cpu.py pins that yardstick to
a numpy model), compared with helpers.assert_results_equal; the reference's goldens where V holds every doc."""
import ctypes as C
import re
import threading

import numpy as np
import pytest

import doc_set_cases as D
import fuzz_cases as F
import helpers as H
import test_gpu_fuzz as TF
from oracle import oracle
from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S

pytestmark = pytest.mark.gpu

LEAN = "scan_simple_valid_kernel"
SWITCH = "PINOT_GPU_SCAN_SIMPLE_VALID"
MAX_STATS_LEFT_OUT = 0.25            # share of fuzz cases whose numEntriesScannedInFilter may come back inexact (filter_entries_exact = 0)


def create(g, mask, fmt):
    mask = np.asarray(mask, dtype=bool)
    return g.create_doc_set(doc_ids=np.flatnonzero(mask).astype(np.int32)) if fmt == "roaring" else g.create_doc_set(words=D.mask_words(mask))


def same_result(a, b):
    assert a.stats == b.stats and a.filter_entries_exact == b.filter_entries_exact and a.group_keys == b.group_keys
    for va, vb in [(a.aggregations, b.aggregations)] + [(a.groups[k], b.groups[k]) for k in a.groups]:
        for x, y in zip(va, vb):
            assert (x.count, x.sum_i64, x.sum_exact) == (y.count, y.sum_i64, y.sum_exact) and x.sum == y.sum
            assert (x.min == y.min or (x.min != x.min and y.min != y.min)) and (x.max == y.max or (x.max != x.max and y.max != y.max))


# ---- the golden segment ----
def golden_group_bys(seg):
    g = H.load_golden_queries()
    ci = seg.column_index
    return [[], [ci("column9")]] + [[ci(c) for c in g[row]["group_by"]] for row in ("inner_segment_group_by_medium", "inner_segment_group_by_large", "inner_segment_group_by_very_large")]


def test_golden_queries_under_a_random_doc_set_in_both_formats(engine):
    seg = H.golden_segment()
    n = seg.num_docs
    mask = np.random.default_rng(11).random(n) < 0.6
    twin = D.twin_segment(seg, [mask])
    vcol = len(seg.columns)
    with engine.open(seg) as g:
        ids = {fmt: create(g, mask, fmt) for fmt in ("roaring", "words")}
        assert all(g.doc_set_cardinality(i) == int(mask.sum()) for i in ids.values()) and ids["roaring"] != ids["words"]
        for user in (H.golden_filter(seg), H.golden_filter(seg, inverted=True), H.golden_filter_physical(seg), None):
            for exclusive in ((False,) if user is not None else (False, True)):
                for group_by in golden_group_bys(seg):
                    per_format = []
                    for fmt, dsid in ids.items():
                        spec = Q.QuerySpec(H.golden_aggregations(seg), filter=D.with_valid(user, Q.leaf(Q.Pred.doc_set(dsid, exclusive))), group_by=group_by)
                        got = g.execute(spec)
                        want = oracle.execute(twin, D.to_twin(spec, {dsid: vcol}))
                        H.assert_results_equal(got, want, check_stats=True)
                        assert got.group_keys == want.group_keys
                        if user is None:
                            assert got.filter_entries_exact and got.stats[1] == 0           # index-only: never left out
                        per_format.append(got)
                    same_result(per_format[0], per_format[1])
                spec = Q.QuerySpec([(Q.COUNT, -1)], filter=D.with_valid(user, Q.leaf(Q.Pred.doc_set(ids["roaring"], exclusive))))
                words, card = g.filter_bitmap(spec)
                owords, ocard = oracle.filter_bitmap(twin, D.to_twin(spec, {ids["roaring"]: vcol}))
                assert card == ocard and np.array_equal(words, owords)
                words2, card2 = g.filter_bitmap(Q.QuerySpec([(Q.COUNT, -1)], filter=D.with_valid(user, Q.leaf(Q.Pred.doc_set(ids["words"], exclusive)))))
                assert card2 == card and np.array_equal(words2, words)
        words, card = g.filter_bitmap(Q.QuerySpec([(Q.COUNT, -1)], filter=Q.leaf(Q.Pred.doc_set(ids["words"]))))
        assert card == int(mask.sum()) and np.array_equal(words, D.mask_words(mask))


def test_all_docs_reproduce_the_goldens_with_scanned_statistics_and_no_docs_give_empty_holders(engine):
    g = H.load_golden_queries()
    seg = H.golden_segment()
    n = seg.num_docs
    ci = seg.column_index
    with engine.open(seg) as gseg:
        for fmt in ("roaring", "words"):
            everything, nothing = create(gseg, np.ones(n, bool), fmt), create(gseg, np.zeros(n, bool), fmt)
            assert gseg.doc_set_cardinality(everything) == n and gseg.doc_set_cardinality(nothing) == 0
            v = Q.leaf(Q.Pred.doc_set(everything))
            res = gseg.execute(Q.QuerySpec(H.golden_aggregations(seg), filter=v))
            H.check_golden_row(res.aggregations, g["inner_segment"]["unfiltered"])            # 30000 / 32317185437847 / ...
            assert list(res.stats) == g["inner_segment"]["unfiltered"]["stats"]
            res = gseg.execute(Q.QuerySpec(H.golden_aggregations(seg), filter=D.with_valid(H.golden_filter_physical(seg), v)))
            H.check_golden_row(res.aggregations, g["inner_segment"]["filtered"])
            assert (res.stats[0], res.stats[2], res.stats[3]) == tuple(g["inner_segment"]["filtered"]["stats"][i] for i in (0, 2, 3))
            gres = gseg.execute(Q.QuerySpec(H.golden_aggregations(seg), filter=v, group_by=[ci("column9")]))
            gw = g["inner_segment_group_by_column9"]["unfiltered"]
            H.check_golden_row(gres.groups[int(np.searchsorted(seg.column("column9").dict_values, gw["key"]))], gw)
            # MetadataAndDictionaryAggregationPlanMakerTest.java:190-209: on the upsert segment max / min(daysSinceEpoch) is an AggregationOperator
            days = ci("daysSinceEpoch")
            spec = Q.QuerySpec([(Q.MAX, days), (Q.MIN, days)], filter=v)
            res = gseg.execute(spec)
            plain = gseg.execute(Q.QuerySpec([(Q.MAX, days), (Q.MIN, days)]))
            assert plain.stats == (n, 0, 0, n) and res.stats == (n, 0, n, n)
            assert res.intermediates() == plain.intermediates()
            # COUNT(*) over the set alone: FastFilteredCountOperator, nothing launched
            res = gseg.execute(Q.QuerySpec([(Q.COUNT, -1)], filter=v))
            assert res.intermediates() == [n] and res.stats == (n, 0, 0, n) and res.dominant_kernel_ms == 0.0
            # the empty set: the empty holders
            e = Q.leaf(Q.Pred.doc_set(nothing))
            for flt in (e, D.with_valid(H.golden_filter(seg), e)):
                res = gseg.execute(Q.QuerySpec(H.golden_aggregations(seg), filter=flt))
                assert res.intermediates() == [0, 0.0, float("-inf"), float("inf"), (0.0, 0)] and res.stats[0] == 0 and res.stats[2] == 0
                assert gseg.execute(Q.QuerySpec(H.golden_aggregations(seg), filter=flt, group_by=[ci("column9")])).groups == {}
            # ... and its flip holds every doc
            res = gseg.execute(Q.QuerySpec(H.golden_aggregations(seg), filter=Q.leaf(Q.Pred.doc_set(nothing, exclusive=True))))
            H.check_golden_row(res.aggregations, g["inner_segment"]["unfiltered"])


# ---- fuzz ----
class StatsTally:
    def __init__(self):
        self.cases = self.left_out = 0

    def add(self, got, want, never_left_out, where):
        self.cases += 1
        if not want.filter_entries_exact:
            return                                   # (the oracle's own count is not the reference's under null handling)
        if got.filter_entries_exact:
            assert got.stats[1] == want.stats[1], "%s: numEntriesScannedInFilter %r != %r" % (where, got.stats, want.stats)
        else:
            assert not never_left_out, "%s: a single-leaf / index-only filter came back without an exact entry count" % where
            self.left_out += 1


def run_typed_fuzz(engine, tally):
    declined = generated = 0
    for seed in F.SEEDS:
        seg = F.make_segment(seed)
        masks = D.fuzz_masks(seg)
        twin = D.twin_fuzz_segment(seg, masks)
        rng = np.random.default_rng(555_000 + F.SEED_BASE + seed)
        with engine.open(seg.data) as g:
            ids = [create(g, masks[0], "roaring"), create(g, masks[1], "words")]
            ran = []
            for qi, fq in enumerate(F.make_queries(seg)):
                dev, shape = D.wrap_fuzz_query(rng, fq, D.device_leaf(ids[0], 0), lambda excl: D.device_leaf(ids[1], 1, excl))
                tw = D.twin_fuzz_query(dev, lambda leaf: D.twin_leaf(len(seg.cols) + leaf.args["which"], leaf.exclusive))
                where = "typed seed %d query %d (%s, n=%d, group_by=%r, null_handling=%r, leaves=%r)" % (seed, qi, shape, seg.n, dev.group_by, dev.null_handling, [x.kind for x in dev.leaves()])
                generated += 1
                try:
                    got = g.execute(dev.spec)
                except _abi.PinotGpuError as e:
                    assert e.status == _abi.PG_ERR_UNSUPPORTED and any(re.search(p, str(e)) for p in F.DECLINE_ALLOW_LIST), "%s: %s" % (where, e)
                    declined += 1
                    continue
                want = oracle.execute(twin.data, tw.spec)
                exp = F.expected(twin, tw)
                try:
                    F.check_result(twin, tw, got, exp)
                    for i, (f, c) in enumerate(tw.aggs):          # ill-conditioned FP sums were held to the model's bound: the helper sees the oracle's figure
                        if f in (Q.SUM, Q.AVG) and c >= 0 and twin.cols[c].pool == "ill":
                            for mine, theirs in [(got.aggregations, want.aggregations)] + [(got.groups[k], want.groups[k]) for k in got.groups if k in want.groups]:
                                if mine:
                                    mine[i].sum = theirs[i].sum
                        # LONG sums: the oracle flags a sum inexact as soon as its int64 side channel wrapped at ANY point of its doc-order
                        # walk, also when the true sum fits an int64 again; the device's modular sum is then the exact sum and it says so.
                        # F.check_result above has held that claim to the model (sum_i64 == the exact integer sum whenever sum_exact): the
                        # helper, which reads an inexact oracle sum as a floating-point one, sees the oracle's figures for such a cell.
                        if f in (Q.SUM, Q.AVG) and c >= 0 and twin.cols[c].kind in (F.DICT_LONG, F.RAW_LONG):
                            for mine, theirs in [(got.aggregations, want.aggregations)] + [(got.groups[k], want.groups[k]) for k in got.groups if k in want.groups]:
                                if mine and mine[i].sum_exact and not theirs[i].sum_exact:
                                    mine[i].sum, mine[i].sum_exact = theirs[i].sum, False
                    H.assert_results_equal(got, want, check_stats=True)
                    assert got.group_keys == want.group_keys and got.num_groups_limit_reached == want.num_groups_limit_reached
                    tally.add(got, want, shape == "single" or D.index_only(dev), where)
                    if not dev.group_by:
                        words, card = g.filter_bitmap(dev.spec)
                        assert card == int(exp.mask.sum()) and np.array_equal(words, F.mask_words(exp.mask)), "filter bitmap"
                except AssertionError as e:
                    raise AssertionError("%s [%s]: %s" % (where, got.dominant_kernel, e)) from e
                ran.append((dev, got))
            for rep in range(2):                                    # the same queries as ONE pg_execute_batch, twice (the second meets the plan cache)
                out = engine.execute_batch([g] * len(ran), [r[0].spec for r in ran]) if ran else []
                for (status, res), (dev, single) in zip(out, ran):
                    assert status == _abi.PG_OK
                    assert res.stats == single.stats and res.group_keys == single.group_keys
                    assert [v.count for v in res.aggregations] == [v.count for v in single.aggregations]
    return generated, declined


def run_dictionary_fuzz(engine, tally):
    """tests/test_gpu_fuzz.py's segments (every packed width) and trees, each behind V at the root and with W at an inner position."""
    for seed in range(24):
        rng = np.random.default_rng(1000 + TF.SEED_BASE + seed)
        n = int(rng.choice([1, 31, 32, 33, 2047, 2048, 2049, 4097, 9001, 20_011]))
        cols = []
        for c in range(3):
            card = int(rng.choice([2, 3, 7, 64, 1000, 5000]))
            natural = max(1, int(np.ceil(np.log2(card))))
            bits = int(rng.integers(natural, 32)) if rng.integers(0, 2) else natural
            cols.append(TF.forced_width_column(rng, "c%d" % c, n, card, bits, affine=bool(rng.integers(0, 2)), with_inverted=(c == 0)))
        seg = S.SegmentData("fuzzv%d" % seed, n, cols)
        masks = [rng.random(n) < float(rng.choice([0.0, 0.02, 0.5, 0.98, 1.0])) for _ in range(2)]
        twin = D.twin_segment(seg, masks)
        with engine.open(seg) as g:
            ids = [create(g, masks[0], "words"), create(g, masks[1], "roaring")]
            column_of = {ids[0]: 3, ids[1]: 4}
            for q in range(12):
                aggs = [(int(f), -1 if f == Q.COUNT else int(rng.integers(0, 3))) for f in rng.choice([Q.COUNT, Q.SUM, Q.MIN, Q.MAX, Q.AVG], int(rng.integers(1, 5)))]
                user = TF.random_tree(rng, seg, n, 2) if rng.integers(0, 5) else None
                shape = "single" if user is None else "root"
                if user is not None and user.op != _abi.PG_FILTER_LEAF and rng.integers(0, 2):
                    k = int(rng.integers(0, len(user.children)))
                    w = Q.leaf(Q.Pred.doc_set(ids[1], exclusive=bool(rng.integers(0, 3) == 0)))
                    user.children[k] = Q.and_(user.children[k], w) if rng.integers(0, 2) else Q.or_(user.children[k], w)
                    shape = "inner"
                group_by = []
                if rng.integers(0, 3) == 0:
                    group_by = [int(x) for x in rng.choice(3, int(rng.integers(1, 3)), replace=False)]
                    if np.prod([seg.columns[x].cardinality for x in group_by]) > 10_000:
                        group_by = group_by[:1]
                spec = Q.QuerySpec(aggs, filter=D.with_valid(user, Q.leaf(Q.Pred.doc_set(ids[0]))), group_by=group_by)
                where = "dictionary seed %d query %d (%s, n=%d)" % (seed, q, shape, n)
                try:
                    got = g.execute(spec)
                except _abi.PinotGpuError as e:
                    assert e.status == _abi.PG_ERR_UNSUPPORTED, "%s: %s" % (where, e)      # more than 8 leaves: a plan-time fallback
                    continue
                tspec = D.to_twin(spec, column_of)
                want = oracle.execute(twin, tspec)
                try:
                    H.assert_results_equal(got, want, check_stats=True)
                    scan_free = all(p.kind in (_abi.PG_PRED_DOC_SET, _abi.PG_PRED_DOC_RANGE, _abi.PG_PRED_MATCH_ALL, _abi.PG_PRED_MATCH_NONE) or p.inverted for p in spec.predicates)
                    tally.add(got, want, shape == "single" or scan_free, where)
                    if not group_by:
                        words, card = g.filter_bitmap(spec)
                        owords, ocard = oracle.filter_bitmap(twin, tspec)
                        assert card == ocard and np.array_equal(words, owords), "filter bitmap"
                except AssertionError as e:
                    raise AssertionError("%s [%s]: %s" % (where, got.dominant_kernel, e)) from e


@pytest.mark.parametrize("cus", [None, "1"], ids=["whole-device", "one-cu"])
def test_fuzz_trees_behind_doc_sets(engine, cus):
    engine.reinit(PINOT_GPU_TEST_CUS=cus)
    tally = StatsTally()
    try:
        generated, declined = run_typed_fuzz(engine, tally)
        run_dictionary_fuzz(engine, tally)
    finally:
        engine.reinit(PINOT_GPU_TEST_CUS=None)
    print("doc-set fuzz: %d cases, %d without an exact entry count, %d of %d typed queries declined" % (tally.cases, tally.left_out, declined, generated))
    assert declined <= 0.10 * generated
    assert tally.cases > 400 and tally.left_out <= MAX_STATS_LEFT_OUT * tally.cases, (tally.left_out, tally.cases)


# ---- the lean kernel ----
LEAN_DOCS = 12_000_037                 # more tiles than resident waves; neither a multiple of 64 nor of 2048
LEAN_BITS = [1, 7, 16, 20]


def lean_segment():
    rng = np.random.default_rng(2026)
    cols = []
    for bits in LEAN_BITS:
        card = 2 if bits == 1 else (1 << bits) - 3
        ids = rng.integers(0, card, LEAN_DOCS).astype(np.int32)
        cols.append(S.Column.from_dict_ids("w%d" % bits, (np.arange(card, dtype=np.int64) * 3 + 1).astype(np.int32), ids))      # affine: summed through the dictId stream
    return S.SegmentData("lean_valid", LEAN_DOCS, cols)


def lean_masks():
    rng = np.random.default_rng(7)
    ends = np.zeros(LEAN_DOCS, bool)
    ends[[0, LEAN_DOCS - 1]] = True
    return [("0%", np.zeros(LEAN_DOCS, bool)), ("0.1%", rng.random(LEAN_DOCS) < 0.001), ("50%", rng.random(LEAN_DOCS) < 0.5),
            ("99.9%", rng.random(LEAN_DOCS) < 0.999), ("100%", np.ones(LEAN_DOCS, bool)), ("first and last", ends)]


def lean_queries(i, seg, valid):
    """(spec builder result, does scan_simple_valid_kernel take it?) for filter column i, aggregated column i + 1."""
    f, a = i, (i + 1) % len(LEAN_BITS)
    card = seg.columns[f].cardinality
    rng_leaf = Q.leaf(Q.Pred.dict_range(f, 0, max(1, card // 3))) if i % 2 == 0 else Q.leaf(Q.Pred.dict_range(f, card // 4, card // 2 + 1, exclusive=(i == 3)))
    return [(Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, a)], filter=Q.and_(rng_leaf, valid)), True),
            (Q.QuerySpec([(Q.MIN, a), (Q.MAX, a), (Q.AVG, a)], filter=Q.and_(valid, rng_leaf)), True),
            (Q.QuerySpec([(Q.COUNT, -1)], filter=Q.and_(rng_leaf, valid)), True),
            (Q.QuerySpec([(Q.SUM, a), (Q.MAX, a)], filter=valid), True),
            (Q.QuerySpec([(Q.SUM, a), (Q.MAX, f)], filter=Q.and_(rng_leaf, valid)), False)]          # two aggregated columns: the general kernel


def test_lean_kernel_switch_on_and_off(engine):
    seg = lean_segment()
    vcol = len(seg.columns)
    with engine.open(seg) as g:
        for label, mask in lean_masks():
            twin = D.twin_segment(seg, [mask])
            dsid = create(g, mask, "roaring" if label in ("0.1%", "first and last", "0%") else "words")
            assert g.doc_set_cardinality(dsid) == int(mask.sum())
            valid = Q.leaf(Q.Pred.doc_set(dsid))
            wanted = {}
            for switch in (None, "0", "2"):
                engine.reinit(**{SWITCH: switch})
                try:
                    for i in range(len(LEAN_BITS)):
                        for qi, (spec, lean) in enumerate(lean_queries(i, seg, valid)):
                            got = g.execute(spec)
                            if (i, qi) not in wanted:
                                wanted[(i, qi)] = oracle.execute(twin, D.to_twin(spec, {dsid: vcol}))
                            want = wanted[(i, qi)]
                            where = "%s docs valid, bits %d, query %d, switch %r: %s" % (label, LEAN_BITS[i], qi, switch, got.dominant_kernel)
                            try:
                                H.assert_results_equal(got, want, check_stats=True)
                            except AssertionError as e:
                                raise AssertionError("%s: %s" % (where, e)) from e
                            assert got.filter_entries_exact and got.stats[1] == want.stats[1], where
                            assert (got.dominant_kernel == LEAN) == (lean and switch != "0"), where
                            if switch == "0":
                                assert got.dominant_kernel in ("scan_private_kernel", "scan_hist_kernel", "scan_agg_kernel"), where
                    # the plain range query on the same segment keeps the headline's kernel
                    plain = g.execute(Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, 1)], filter=Q.leaf(Q.Pred.dict_range(3, 0, 1000))))
                    assert plain.dominant_kernel == "scan_simple_kernel", plain.dominant_kernel
                finally:
                    engine.reinit(**{SWITCH: None})
            g.release_doc_set(dsid)


# ---- lifetime ----
def small_segment(n=300_017, seed=5):
    rng = np.random.default_rng(seed)
    v = S.Column.from_dict_ids("v", (np.arange(5000, dtype=np.int64) * 7 + 3).astype(np.int32), rng.integers(0, 5000, n).astype(np.int32))
    f = S.Column.from_dict_ids("f", np.arange(1000, dtype=np.int32), rng.integers(0, 1000, n).astype(np.int32))
    k = S.Column.from_dict_ids("k", np.arange(40, dtype=np.int32), rng.integers(0, 40, n).astype(np.int32))
    return S.SegmentData("life%d" % seed, n, [v, f, k])


def status_of(g, spec):
    res = _abi.pg_result()
    st = int(g.lib.pg_execute(g.handle, C.byref(spec.c), C.byref(res)))
    g.lib.pg_result_free(C.byref(res))
    return st


def test_release_refuses_the_id_frees_the_bytes_and_drops_cached_queries(engine):
    seg = small_segment()
    n = seg.num_docs
    mask = np.random.default_rng(1).random(n) < 0.4
    bitmap_bytes = ((n + 2047) // 2048) * 256
    with engine.open(seg) as g:
        before = g.device_bytes()
        dsid = create(g, mask, "roaring")
        assert g.device_bytes() == before + bitmap_bytes
        headline = Q.QuerySpec([(Q.SUM, 0)], filter=Q.and_(Q.leaf(Q.Pred.dict_range(1, 0, 100)), Q.leaf(Q.Pred.doc_set(dsid))))
        grouped = Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, 0)], filter=Q.leaf(Q.Pred.doc_set(dsid)), group_by=[2])      # the one-launch group-by: its lowering is cached
        first = [g.execute(headline), g.execute(grouped)]
        again = [g.execute(headline), g.execute(grouped)]
        batch = engine.execute_batch([g, g], [headline, grouped])
        batch2 = engine.execute_batch([g, g], [headline, grouped])                # meets the plan cache
        for a, b, (st1, c), (st2, d) in zip(first, again, batch, batch2):
            assert st1 == st2 == _abi.PG_OK
            same_result(a, b), same_result(a, c), same_result(a, d)
        assert first[1].stats[0] == int(mask.sum())
        after_queries = g.device_bytes()
        g.release_doc_set(dsid)
        assert g.device_bytes() == after_queries - bitmap_bytes
        for spec in (headline, grouped, Q.QuerySpec([(Q.COUNT, -1)], filter=Q.leaf(Q.Pred.doc_set(dsid)))):
            assert g.check(spec) == _abi.PG_ERR_INVALID_ARGUMENT and status_of(g, spec) == _abi.PG_ERR_INVALID_ARGUMENT
            assert "doc set" in g.lib.pg_last_error().decode()
        for st, _ in engine.execute_batch([g, g], [headline, grouped]):
            assert st == _abi.PG_ERR_INVALID_ARGUMENT
        with pytest.raises(_abi.PinotGpuError):
            g.release_doc_set(dsid)
        with pytest.raises(_abi.PinotGpuError):
            g.doc_set_cardinality(dsid)
        with pytest.raises(_abi.PinotGpuError):
            g.filter_bitmap(headline)
        # ids are never reused, and a set of another segment is unknown here
        newer = create(g, mask, "words")
        assert newer > dsid
        with engine.open(small_segment(seed=6)) as other:
            foreign = create(other, mask, "words")
            assert foreign > newer and status_of(g, Q.QuerySpec([(Q.COUNT, -1)], filter=Q.leaf(Q.Pred.doc_set(foreign)))) == _abi.PG_ERR_INVALID_ARGUMENT
        same_result(g.execute(Q.QuerySpec([(Q.SUM, 0)], filter=Q.and_(Q.leaf(Q.Pred.dict_range(1, 0, 100)), Q.leaf(Q.Pred.doc_set(newer))))), first[0])
    with engine.open(seg) as g:                # close frees what was not released
        create(g, mask, "words")


def test_bad_doc_sets_are_refused(engine):
    seg = small_segment(n=70_001)
    n = seg.num_docs
    with engine.open(seg) as g:
        words = np.zeros((n + 63) // 64, dtype=np.uint64)
        for bad in (words[:-1], np.concatenate([words, words[:1]])):
            with pytest.raises(_abi.PinotGpuError) as e:
                g.create_doc_set(words=bad)
            assert e.value.status == _abi.PG_ERR_INVALID_ARGUMENT
        beyond = words.copy()
        beyond[-1] = np.uint64(1) << np.uint64(n & 63)             # docId n: the first one past the segment
        with pytest.raises(_abi.PinotGpuError) as e:
            g.create_doc_set(words=beyond)
        assert e.value.status == _abi.PG_ERR_INVALID_ARGUMENT
        for ids in ([0, 5, n], [n - 1, 70_000 + 65_536], list(range(60_000, n + 1))):
            with pytest.raises(_abi.PinotGpuError) as e:
                g.create_doc_set_raw(_abi.PG_DOC_SET_ROARING, S.roaring_serialize(np.array(ids, dtype=np.int32), None))
            assert e.value.status == _abi.PG_ERR_INVALID_ARGUMENT, ids
        for raw in (np.zeros(3, np.uint8), np.full(64, 0xAB, np.uint8)):
            with pytest.raises(_abi.PinotGpuError) as e:
                g.create_doc_set_raw(_abi.PG_DOC_SET_ROARING, raw)
            assert e.value.status == _abi.PG_ERR_INVALID_ARGUMENT
        with pytest.raises(_abi.PinotGpuError):
            g.create_doc_set_raw(5, words.view(np.uint8))
        last = g.create_doc_set(doc_ids=[n - 1])                     # the last doc is fine, in every container kind
        runs = g.create_doc_set(doc_ids=np.arange(100, n, dtype=np.int32))
        assert g.doc_set_cardinality(last) == 1 and g.doc_set_cardinality(runs) == n - 100
        res = g.execute(Q.QuerySpec([(Q.COUNT, -1), (Q.MAX, 0)], filter=Q.leaf(Q.Pred.doc_set(runs))))
        assert res.aggregations[0].count == n - 100


def test_two_doc_sets_used_concurrently_each_give_their_own_answer(engine):
    seg = small_segment(n=2_000_003, seed=8)
    n = seg.num_docs
    rng = np.random.default_rng(3)
    masks = [rng.random(n) < 0.3, rng.random(n) < 0.8]
    with engine.open(seg) as g:
        ids = [create(g, masks[0], "roaring"), create(g, masks[1], "words")]
        twins = [D.twin_segment(seg, [m]) for m in masks]
        specs = [Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, 0)], filter=Q.and_(Q.leaf(Q.Pred.dict_range(1, 100, 700)), Q.leaf(Q.Pred.doc_set(i)))) for i in ids]
        wants = [oracle.execute(twins[k], D.to_twin(specs[k], {ids[k]: 3})) for k in range(2)]
        errors = []

        def worker(k):
            try:
                for _ in range(25):
                    H.assert_results_equal(g.execute(specs[k]), wants[k], check_stats=True)
            except Exception as e:          # noqa: BLE001
                errors.append((k, e))
        threads = [threading.Thread(target=worker, args=(k % 2,)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert wants[0].aggregations[0].count != wants[1].aggregations[0].count


def test_batch_over_eight_segments_each_with_its_own_doc_set(engine):
    segs = [small_segment(n=100_003 + 4099 * s, seed=20 + s) for s in range(8)]
    opened = [engine.open(s) for s in segs]
    try:
        rng = np.random.default_rng(9)
        masks = [rng.random(s.num_docs) < (0.1 + 0.1 * k) for k, s in enumerate(segs)]
        ids = [create(g, m, "roaring" if k % 2 else "words") for k, (g, m) in enumerate(zip(opened, masks))]
        for make in (lambda v: Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, 0)], filter=Q.and_(Q.leaf(Q.Pred.dict_range(1, 0, 100)), v)),
                     lambda v: Q.QuerySpec([(Q.COUNT, -1)], filter=v),
                     lambda v: Q.QuerySpec([(Q.SUM, 0), (Q.MIN, 1)], filter=Q.or_(Q.leaf(Q.Pred.dict_range(1, 0, 100)), Q.not_(v))),
                     lambda v: Q.QuerySpec([(Q.COUNT, -1), (Q.MAX, 0)], filter=v, group_by=[2])):
            specs = [make(Q.leaf(Q.Pred.doc_set(i))) for i in ids]
            singles = [g.execute(s) for g, s in zip(opened, specs)]
            for rep in range(2):
                for k, (st, res) in enumerate(engine.execute_batch(opened, specs)):
                    assert st == _abi.PG_OK
                    same_result(res, singles[k])
            for k in (0, 7):
                H.assert_results_equal(singles[k], oracle.execute(D.twin_segment(segs[k], [masks[k]]), D.to_twin(specs[k], {ids[k]: 3})), check_stats=True)
    finally:
        for g in opened:
            g.close()


def test_the_jni_harness_path(engine):
    """What GpuSegment.docSetFor / GpuQueryLowering do, through the JNI functions run by the JVM stand-in: create the doc set from a direct
    buffer, lower AND(filter, valid docs), queryCheck, execute, executeBatch, release."""
    from pinot_amd import jni_harness as J
    from pinot_amd import marshal as M
    jvm = J.FakeJvm()
    jvm.call("init", None, C.c_int32(0), C.c_int32(0))
    try:
        seg = H.golden_segment()
        n = seg.num_docs
        mask = np.random.default_rng(21).random(n) < 0.7
        twin = D.twin_segment(seg, [mask])
        refs_before = jvm.lib.fj_live_refs()
        handle = jvm.segment_open(seg)
        try:
            bytes_before = jvm.call("segmentDeviceBytes", C.c_int64, C.c_int64(handle))
            dsid = jvm.doc_set_create(handle, _abi.PG_DOC_SET_ROARING, S.roaring_serialize(np.flatnonzero(mask).astype(np.int32), n))
            assert jvm.doc_set_cardinality(handle, dsid) == int(mask.sum())
            assert jvm.call("segmentDeviceBytes", C.c_int64, C.c_int64(handle)) == bytes_before + ((n + 2047) // 2048) * 256
            specs = [Q.QuerySpec(H.golden_aggregations(seg), filter=D.with_valid(flt, Q.leaf(Q.Pred.doc_set(dsid))), group_by=gb)
                     for flt in (None, H.golden_filter_physical(seg)) for gb in ([], [seg.column_index("column9")])]
            for spec in specs:
                assert jvm.query_check(handle, spec) == _abi.PG_OK
                got = jvm.execute(handle, spec)
                want = oracle.execute(twin, D.to_twin(spec, {dsid: len(seg.columns)}))
                assert list(got[0][:4]) == list(want.stats) and got[0][M.H_FILTER_ENTRIES_EXACT] == 1
                if not spec.group_by:
                    assert int(got[2][0]) == want.aggregations[0].count and int(got[4][1]) == want.aggregations[1].sum_i64
                else:
                    assert sorted(got[1].tolist()) == sorted(want.groups)
            jvm.doc_set_release(handle, dsid)
            assert jvm.call("segmentDeviceBytes", C.c_int64, C.c_int64(handle)) == bytes_before
            with pytest.raises(J.JavaException) as e:
                jvm.execute(handle, specs[0])
            assert e.value.cls == "java/lang/RuntimeException" and "doc set" in e.value.message
            with pytest.raises(J.JavaException):
                jvm.doc_set_release(handle, dsid)
        finally:
            jvm.call("segmentClose", None, C.c_int64(handle))
        assert jvm.lib.fj_pins() == 0 and jvm.lib.fj_live_refs() == refs_before
    finally:
        engine.reinit()


def test_sql_over_host_segments_with_queryable_doc_ids(engine):
    """ph_execute_sql over four segments of an upsert table, each with its own valid docs: every segment's block and the combined result
    equal the oracle twins' (merged the way the combine operator merges: counts and sums add, MAX / MIN fold)."""
    from pinot_amd import host
    host.init_plan_maker(device=0, time_kernels=True)
    data = H.golden_segment()
    n = data.num_docs
    rng = np.random.default_rng(31)
    masks = [rng.random(n) < d for d in (0.9, 0.5, 0.05, 1.0)]
    segs = [host.HostSegment(data, string_dicts=data.string_dicts) for _ in masks]
    try:
        for s, m in zip(segs, masks):
            s.set_queryable_doc_ids(m)
        ci = data.column_index
        aggs = [(Q.COUNT, -1), (Q.SUM, ci("column1")), (Q.MAX, ci("column3")), (Q.MIN, ci("column6"))]
        sql = "SELECT COUNT(*), SUM(column1), MAX(column3), MIN(column6) FROM testTable"
        where = " WHERE column1 > 100000000 AND column3 BETWEEN 20000000 AND 1000000000"
        user = Q.and_(Q.leaf(H.range_pred(data, "column1", lower=100000000, lower_inclusive=False)), Q.leaf(H.range_pred(data, "column3", lower=20000000, upper=1000000000)))
        for text, flt in ((sql, None), (sql + where, user)):
            out = host.execute_sql(segs, text, max_execution_threads=4)
            wants = [oracle.execute(D.twin_segment(data, [m]), Q.QuerySpec(aggs, filter=D.with_valid(flt, Q.leaf(D.twin_pred(len(data.columns)))))) for m in masks]
            for block, want in zip(out["segments"], wants):
                assert block["intermediate"] == [want.aggregations[0].count, want.aggregations[1].sum, want.aggregations[2].max, want.aggregations[3].min]
                st = block["stats"]
                assert (st["numDocsScanned"], st["numEntriesScannedPostFilter"], st["numTotalDocs"]) == (want.stats[0], want.stats[2], want.stats[3])
                if flt is None:
                    assert st["numEntriesScannedInFilter"] == 0
            total = 0.0
            for w in wants:
                total = total + w.aggregations[1].sum               # SumAggregationFunction.merge: double '+', segment order
            assert out["combined"]["intermediate"] == [sum(w.aggregations[0].count for w in wants), total, max(w.aggregations[2].max for w in wants), min(w.aggregations[3].min for w in wants)]
        # COUNT(*) alone: each segment answers with its set's cardinality (FastFilteredCountOperator)
        out = host.execute_sql(segs, "SELECT COUNT(*) FROM testTable")
        assert [b["intermediate"][0] for b in out["segments"]] == [int(m.sum()) for m in masks]
        assert all(b["stats"]["numEntriesScannedPostFilter"] == 0 for b in out["segments"])
        # group-by behind the valid docs, and a replaced snapshot
        segs[0].set_queryable_doc_ids([0, 1, 2])                     # FilterPlanNodeTest: three matching docs
        out = host.execute_sql(segs[:1], "SELECT COUNT(*) FROM testTable")
        assert out["segments"][0]["intermediate"] == [3]
        groups = host.execute_sql(segs[:1], "SELECT COUNT(*) FROM testTable GROUP BY column9 LIMIT 100000")["segments"][0]["groups"]
        assert sum(r["intermediate"][0] for r in groups) == 3
        segs[0].set_queryable_doc_ids(None)
        assert host.execute_sql(segs[:1], "SELECT COUNT(*) FROM testTable")["segments"][0]["intermediate"] == [n]
        with pytest.raises(host.HostError):
            segs[0].set_queryable_doc_ids([n])                       # a docId beyond the segment is refused when it reaches the device
        assert host.execute_sql(segs[:1], "SELECT COUNT(*) FROM testTable")["segments"][0]["intermediate"] == [n]
    finally:
        for s in segs:
            s.destroy()
        engine.reinit()
