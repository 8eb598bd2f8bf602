"""CPU tier of the doc-set feature (PG_PRED_DOC_SET, pg_doc_set_*): the yardstick the GPU tier uses -- the oracle over the twin segment
of tests/doc_set_cases.py -- against a numpy model, the C ABI's error paths without a device, and FilterPlanNodeTest as a case."""
import ctypes as C

import numpy as np
import pytest

import doc_set_cases as D
import fuzz_cases as F
import helpers as H
from oracle import oracle
from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S


def wrapped(seed):
    """The typed fuzz's segment and queries of `seed`, every tree behind V at the root (and W inside, where there is room): the device's
    form (Pred.doc_set with ids 1 and 2, as a device would hand them out) and its rewriting for the twin."""
    seg = F.make_segment(seed)
    masks = D.fuzz_masks(seg)
    twin = D.twin_fuzz_segment(seg, masks)
    rng = np.random.default_rng(555_000 + F.SEED_BASE + seed)
    out = []
    for fq in F.make_queries(seg):
        dev, shape = D.wrap_fuzz_query(rng, fq, D.device_leaf(1, 0), lambda excl: D.device_leaf(2, 1, excl))
        tw = D.twin_fuzz_query(dev, lambda leaf: D.twin_leaf(len(seg.cols) + leaf.args["which"], leaf.exclusive))
        out.append((fq, dev, tw, shape))
    return seg, masks, twin, out


@pytest.mark.parametrize("seed", F.SEEDS)
def test_the_oracle_twin_equals_the_numpy_model(seed):
    """AND(tree, V) over the twin: docs, aggregates, numDocsScanned and the entries post filter are the exact model's (fuzz_cases.expected
    over the twin), and the docs are the user's filter mask restricted to V -- also under null handling, where V has no NULL set."""
    seg, masks, twin, queries = wrapped(seed)
    for qi, (fq, dev, tw, shape) in enumerate(queries):
        assert any(p.kind == _abi.PG_PRED_DOC_SET for p in dev.spec.predicates)
        assert not any(p.kind == _abi.PG_PRED_DOC_SET for p in tw.spec.predicates)
        got = oracle.execute(twin.data, tw.spec)
        exp = F.expected(twin, tw)
        try:
            F.check_result(twin, tw, got, exp)
            if shape != "inner":
                assert np.array_equal(exp.mask, F.filter_mask(seg, fq) & masks[0])
            words, card = oracle.filter_bitmap(twin.data, tw.spec)
            assert card == int(exp.mask.sum()) and np.array_equal(words, F.mask_words(exp.mask))
            if not tw.group_by and not tw.null_handling:
                assert got.stats[0] == int(exp.mask.sum())
                projected = len({c for f, c in tw.aggs if f != Q.COUNT})
                assert got.stats[2] == int(exp.mask.sum()) * projected and got.stats[3] == seg.n
            if D.index_only(dev) and not tw.null_handling:           # (the oracle's count is the reference's only without null handling)
                assert got.stats[1] == 0 and got.filter_entries_exact
        except AssertionError as e:
            raise AssertionError("seed %d query %d (%s, n=%d, leaves=%r): %s" % (seed, qi, shape, seg.n, [x.kind for x in dev.leaves()], e)) from e


def test_to_twin_rewrites_a_query_spec():
    v = Q.Pred.doc_set(7)
    spec = Q.QuerySpec([(Q.COUNT, -1)], filter=Q.and_(Q.leaf(Q.Pred.dict_range(0, 1, 3)), Q.or_(Q.leaf(v), Q.not_(Q.leaf(v))), Q.leaf(Q.Pred.doc_set(9, exclusive=True))))
    assert [p.kind for p in spec.predicates] == [_abi.PG_PRED_DICT_RANGE, _abi.PG_PRED_DOC_SET, _abi.PG_PRED_DOC_SET]
    assert spec.predicates[1].lo == 7 and spec.predicates[2].lo == 9 and spec.c.predicates[2].exclusive == 1 and spec.c.predicates[1].lo == 7
    twin = D.to_twin(spec, {7: 4, 9: 5})
    assert [(p.kind, p.column, p.lo, p.hi, p.exclusive, p.inverted) for p in twin.predicates] == [
        (_abi.PG_PRED_DICT_RANGE, 0, 1, 3, False, False), (_abi.PG_PRED_DICT_RANGE, 4, 1, 2, False, True), (_abi.PG_PRED_DICT_RANGE, 5, 1, 2, True, True)]
    assert twin.c.num_filter_nodes == spec.c.num_filter_nodes == 7


def test_fast_filtered_count_and_scanned_min_max_on_the_twin():
    """The plan rules the engine has to reproduce, read off the oracle: COUNT(*) under V alone is V's cardinality with statistics
    (card, 0, 0, totalDocs); MIN / MAX of a dictionary column under V = all docs is SCANNED (numEntriesScannedPostFilter = numDocs),
    not answered from the dictionary like the same query on a segment without queryable docIds
    (MetadataAndDictionaryAggregationPlanMakerTest.java:190-209)."""
    n = 5000
    rng = np.random.default_rng(4)
    col = S.Column.dict_encoded("v", rng.integers(0, 900, n).astype(np.int32))
    seg = S.SegmentData("upsert", n, [col])
    for mask in (rng.random(n) < 0.3, np.ones(n, bool), np.zeros(n, bool)):
        twin = D.twin_segment(seg, [mask])
        card = int(mask.sum())
        got = oracle.execute(twin, Q.QuerySpec([(Q.COUNT, -1)], filter=Q.leaf(D.twin_pred(1))))
        assert got.aggregations[0].count == card and got.stats == (card, 0, 0, n)
        got = oracle.execute(twin, Q.QuerySpec([(Q.MIN, 0), (Q.MAX, 0)], filter=Q.leaf(D.twin_pred(1))))
        assert got.stats == (card, 0, card, n)
    plain = oracle.execute(seg, Q.QuerySpec([(Q.MIN, 0), (Q.MAX, 0)]))
    assert plain.stats == (n, 0, 0, n)


def test_filter_plan_node_test_as_a_case():
    """FilterPlanNodeTest.java:56-76: the queryable docIds are {0, 1, 2}; the segment is looked at again and again while it grows under the
    same set, and the filter always matches exactly 3 docs."""
    valid = np.array([0, 1, 2])
    for n in (3, 4, 10, 2047, 2048, 2049, 70_000):
        mask = np.zeros(n, bool)
        mask[valid] = True
        seg = S.SegmentData("growing", n, [S.Column.dict_encoded("c", np.arange(n, dtype=np.int32) % 7)])
        twin = D.twin_segment(seg, [mask])
        spec = D.to_twin(Q.QuerySpec([(Q.COUNT, -1)], filter=D.with_valid(None, Q.leaf(Q.Pred.doc_set(1)))), {1: 1})
        got = oracle.execute(twin, spec)
        assert got.aggregations[0].count == 3 and got.stats == (3, 0, 0, n)
        words, card = oracle.filter_bitmap(twin, spec)
        assert card == 3 and np.array_equal(np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")[:n]), valid)
        spec = D.to_twin(Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, 0)], filter=D.with_valid(Q.leaf(Q.Pred.dict_range(0, 0, 7)), Q.leaf(Q.Pred.doc_set(1)))), {1: 1})
        got = oracle.execute(twin, spec)
        assert got.aggregations[0].count == 3 and got.aggregations[1].sum_i64 == 3


def test_doc_set_calls_fail_with_a_status_and_a_message_without_a_device():
    """Before pg_init every doc-set entry point answers PG_ERR_NOT_INITIALIZED; null arguments give a status and a message, never an abort."""
    lib = _abi.load_gpu_library()
    assert _abi.PG_ABI_VERSION == 5 and _abi.PG_PRED_DOC_SET == 8 and (_abi.PG_DOC_SET_ROARING, _abi.PG_DOC_SET_WORDS) == (0, 1)
    out = C.c_int64(-1)
    words = np.zeros(4, dtype=np.uint64)
    fake = C.c_void_p(0)
    for st in (lib.pg_doc_set_create(fake, _abi.PG_DOC_SET_WORDS, words.ctypes.data_as(C.c_void_p), words.nbytes, C.byref(out)),
               lib.pg_doc_set_create(fake, _abi.PG_DOC_SET_WORDS, None, 8, None),
               lib.pg_doc_set_create(fake, 7, None, 0, C.byref(out)),
               lib.pg_doc_set_release(fake, 1),
               lib.pg_doc_set_cardinality(fake, 1, C.byref(out)),
               lib.pg_doc_set_cardinality(fake, 1, None)):
        assert st in (_abi.PG_ERR_NOT_INITIALIZED, _abi.PG_ERR_INVALID_ARGUMENT), st
        assert lib.pg_last_error()
    assert out.value == -1


def test_doc_set_calls_before_pg_init_are_refused_in_a_fresh_process():
    import os
    import subprocess
    import sys
    code = ("import ctypes as C\nfrom pinot_amd import _abi\nlib = _abi.load_gpu_library()\nout = C.c_int64(0)\n"
            "print(lib.pg_doc_set_create(None, 1, None, 0, C.byref(out)), lib.pg_doc_set_release(None, 1), lib.pg_doc_set_cardinality(None, 1, C.byref(out)))\n"
            "print(lib.pg_last_error().decode())\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proc = subprocess.run([sys.executable, "-c", code], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    lines = proc.stdout.decode().splitlines()
    assert proc.returncode == 0 and lines[0].split() == [str(_abi.PG_ERR_NOT_INITIALIZED)] * 3 and "pg_init" in lines[1], (lines, proc.stderr.decode()[-500:])


def test_the_predicate_round_trips_through_the_marshalling():
    """The flat arrays GpuQueryLowering writes (jni/pg_marshal.h) carry PG_PRED_DOC_SET like every kind: the id in the predicate's first
    long, `exclusive` in its ints."""
    from pinot_amd import marshal as M
    from test_marshal import same_query
    big = (1 << 40) + 12345                                   # ids are 64-bit
    spec = Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, 0)], filter=Q.and_(Q.leaf(Q.Pred.dict_range(1, 2, 9)), Q.leaf(Q.Pred.doc_set(big)), Q.not_(Q.leaf(Q.Pred.doc_set(3, exclusive=True)))),
                       group_by=[2], null_handling=True)
    flat = M.flatten(spec)
    assert list(flat["pred_ints"][4:8]) == [_abi.PG_PRED_DOC_SET, 0, _abi.PG_EVAL_SCAN, 0] and list(flat["pred_longs"][2:4]) == [big, 0]
    assert list(flat["pred_ints"][8:12]) == [_abi.PG_PRED_DOC_SET, 0, _abi.PG_EVAL_SCAN, 1] and flat["pred_longs"][4] == 3
    with M.MarshalledQuery(spec) as mq:
        same_query(mq.c, spec.c)
        assert mq.c.predicates[1].kind == _abi.PG_PRED_DOC_SET and mq.c.predicates[1].lo == big


def test_the_jni_doc_set_functions_map_statuses_to_exceptions_and_leave_nothing_pinned():
    """docSetCreate / docSetRelease / docSetCardinality through the JVM stand-in, before pg_init: RuntimeException carrying pg_last_error;
    a buffer that is not direct: IllegalArgumentException; no local reference or pin is left behind."""
    from pinot_amd import jni_harness as J
    jvm = J.FakeJvm()
    before = jvm.lib.fj_live_refs()
    data = S.roaring_serialize(np.array([0, 1, 2], dtype=np.int32), None)
    for call in (lambda: jvm.doc_set_create(0, _abi.PG_DOC_SET_ROARING, data), lambda: jvm.doc_set_release(0, 1), lambda: jvm.doc_set_cardinality(0, 1)):
        with pytest.raises(J.JavaException) as e:
            call()
        assert e.value.cls == "java/lang/RuntimeException" and e.value.message
    with pytest.raises(J.JavaException) as e:
        jvm.call("docSetCreate", C.c_int64, C.c_int64(0), C.c_int32(0), None, C.c_int64(8))
    assert e.value.cls == "java/lang/IllegalArgumentException"
    assert jvm.lib.fj_pins() == 0 and jvm.lib.fj_live_refs() == before


def test_the_host_mirror_wraps_every_filter_like_filter_plan_node():
    """FilterPlanNode.java:88-106 read back with ph_explain_filter (no device): with queryable docIds the plan is getAndFilterOperator(
    [user filter, valid docs]) -- children by priority: sorted (0) < the bitmap (100) < AND (300) < OR (400) < scans (500); a user AND stays
    a child of its own (the reference does not flatten it) --, the leaf alone without a filter; Empty / MatchAll user filters fold as ever."""
    from pinot_amd import host
    from test_host_mirror_cpu import _plan_segment
    seg = _plan_segment()
    ex = lambda where: host.explain_filter(seg, "SELECT COUNT(*) FROM planSegment" + (" WHERE " + where if where else ""))
    valid = "BITMAP(queryableDocIds)"
    try:
        assert ex("") == "MATCH_ALL" and ex("scan > 5") == "SCAN(scan dictIds 6..99)"
        seg.set_queryable_doc_ids([0, 1, 2])
        assert ex("") == valid
        assert ex("scan > 5") == "AND(" + valid + ", SCAN(scan dictIds 6..99))"
        assert ex("s = 7") == "AND(SORTED(s docs 70..79), " + valid + ")"
        assert ex("n IS NULL") == "AND(BITMAP(n IS NULL), " + valid + ")"                      # equal priorities keep the list's order: filter, then valid docs
        assert ex("scan > 5 AND scan < 50") == "AND(" + valid + ", AND(SCAN(scan dictIds 6..99), SCAN(scan dictIds 0..49)))"
        assert ex("scan > 5 OR inv = 3") == "AND(" + valid + ", OR(SCAN(scan dictIds 6..99), INVERTED(inv dictIds 3..3)))"
        assert ex("inv = 999") == "EMPTY" and ex("inv != 999") == valid
        seg.set_queryable_doc_ids(np.arange(1000) % 3 == 0)                                  # a new snapshot replaces the old one
        assert ex("scan > 5") == "AND(" + valid + ", SCAN(scan dictIds 6..99))"
        seg.set_queryable_doc_ids(None)
        assert ex("") == "MATCH_ALL" and ex("scan > 5") == "SCAN(scan dictIds 6..99)"
        # a segment that is not on a device is declined with a message, as before
        seg.set_queryable_doc_ids([5])
        with pytest.raises(host.HostError) as e:
            host.execute_sql([seg], "SELECT COUNT(*) FROM planSegment")
        assert "not loaded" in str(e.value)
    finally:
        seg.destroy()
