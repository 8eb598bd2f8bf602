"""The Roaring decoders of the device -- index_and_kernel / index_and_batch_kernel (pinot_amd/csrc/pg_index_and.h), roaring_expand_kernel
(pg_kernels.h) behind inverted leaves under OR / NOT, dense AND children, doc sets and null value vectors, and parse_roaring's directory
(pg_engine.hip) -- on the constructed corpus of tests/roaring_cases.py: every container kind at every byte lead, the array piece and
scatter edges, multi-run containers, window presence patterns, exclusive members at three tail lengths.

Every query's answer equals the numpy model exactly and the oracle field for field with its statistics, the filter bitmap equals the
model's words, a second execution gives the same answer, and no query may be declined: a PinotGpuError fails the test.  The expected
values are computed once per segment and shared by every grid setting (tests/test_roaring_cases_cpu.py pins oracle == model)."""
import os

import numpy as np
import pytest

from oracle import oracle
from pinot_amd import _abi
import helpers as H
import roaring_cases as RC

pytestmark = pytest.mark.gpu

CUS, WAVES, GATHER = "PINOT_GPU_TEST_CUS", "PINOT_GPU_INDEX_AND_WAVES", "PINOT_GPU_INDEX_GATHER"
GRIDS = {
    "defaults": {},
    "one_wave": {CUS: 1, WAVES: 1},                # one wave walks every window, every container kind after every other
    "two_waves": {CUS: 1, WAVES: 2},               # two waves, alternating windows
    "wave_per_window": {WAVES: -1},                # no look-ahead
    "no_gather": {GATHER: 0},                      # the bitmap -> scan path for the sparse shapes too
}

_WANT = {}


def expected(seg, queries, tag):
    """[(model, oracle result)] per query and {label: (oracle words, cardinality)}, computed once per (segment, build, list)."""
    k = (seg.key, seg.run_optimize, tag)
    if k not in _WANT:
        rows, bitmaps = [], {}
        for q in queries:
            rows.append((RC.model(seg, q), oracle.execute(seg.data, q.spec(seg))))
            if q.label not in bitmaps:
                bitmaps[q.label] = oracle.filter_bitmap(seg.data, q.bitmap_spec(seg))
        _WANT[k] = (rows, bitmaps)
    return _WANT[k]


class switches:
    """Environment switches for the length of a `with` (PINOT_GPU_TEST_CUS is read when a segment opens: open inside)."""

    def __init__(self, engine, env):
        self.engine, self.env = engine, env

    def __enter__(self):
        self.had = {k: os.environ.get(k) for k in self.env}
        self.engine.reinit(**self.env)

    def __exit__(self, *exc):
        self.engine.reinit(**self.had)


def answer(res):
    rows = [("", res.aggregations)] + sorted(res.groups.items(), key=lambda kv: kv[0])
    return res.stats, res.filter_entries_exact, [(k, [(a.count, a.sum_i64, a.sum, a.min, a.max) for a in v]) for k, v in rows]


def run_corpus(engine, seg, queries, tag, env):
    """Every query of the list on one open segment; returns (queries executed, {dominant kernels of the index-led SUM(v) lists})."""
    rows, bitmaps = expected(seg, queries, tag)
    gather_on = str(env.get(GATHER, 1)) != "0"
    executed, kernels, checked = 0, set(), set()
    with switches(engine, env):
        with engine.open(seg.data) as g:
            doc_sets = {}
            for q in queries:
                for col, name in q.doc_sets:
                    if (col, name) not in doc_sets:
                        docs = np.flatnonzero(seg.ids[col] == seg.dict_id(col, name)).astype(np.int32)
                        doc_sets[(col, name)] = g.create_doc_set(doc_ids=docs)
                        assert g.doc_set_cardinality(doc_sets[(col, name)]) == docs.shape[0]
            for q, (want, ref) in zip(queries, rows):
                where = "%s/%s %s" % (seg.key, "runs" if seg.run_optimize else "plain", tag)
                spec = q.spec(seg, doc_sets)
                got = g.execute(spec)                                        # (a decline raises PinotGpuError: there is no allow-list)
                RC.assert_matches_model(got, want, q, where)
                H.assert_results_equal(got, ref, check_stats=True)
                assert sorted(got.group_keys) == sorted(ref.group_keys), (where, q.label)
                if q.index_led and (q.aggs == RC.COUNT_ONLY or (gather_on and q.certainly_gathered(seg))):
                    assert got.dominant_kernel == "index_and_kernel", (where, q.label, q.aggs, got.dominant_kernel)
                if q.index_led and not q.group_by and q.aggs in (RC.SUM_V, RC.FIVE_V):
                    kernels.add(got.dominant_kernel)
                if q.label not in checked:
                    checked.add(q.label)
                    words, card = g.filter_bitmap(q.bitmap_spec(seg, doc_sets))
                    assert card == want["count"] and np.array_equal(words, RC.mask_words(want["mask"])), (where, q.label)
                    assert card == bitmaps[q.label][1] and np.array_equal(words, bitmaps[q.label][0]), (where, q.label)
                assert answer(g.execute(spec)) == answer(got), (where, q.label)      # the counter lines were re-zeroed behind the first answer
                executed += 1
            for dsid in doc_sets.values():
                g.release_doc_set(dsid)
    return executed, kernels


@pytest.mark.parametrize("run_optimize", [True, False], ids=["runs", "plain"])
@pytest.mark.parametrize("key", RC.SINGLE)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_corpus(engine, grid, key, run_optimize):
    seg = RC.segment(key, run_optimize)
    queries = RC.queries(seg)
    executed, kernels = run_corpus(engine, seg, queries, "corpus", GRIDS[grid])
    assert executed == len(queries) and executed > 150
    print("corpus %s/%s under %s: %d queries, 0 declined" % (key, "runs" if run_optimize else "plain", grid, executed))
    if key == "main" and grid != "no_gather":
        # the gathered side of the rule occurs (run_corpus asserts the kernel of every shape that is certainly gathered); the other side
        # is `b.every & a.filler`, ~39 000 expected docs against 24 (test_the_aggregation_lists_meet_both_sides_of_the_gather_rule):
        # its dominant kernel is whichever of the two launches took longer, so it is not asserted by name
        assert "index_and_kernel" in kernels, kernels


@pytest.mark.parametrize("run_optimize", [True, False], ids=["runs", "plain"])
@pytest.mark.parametrize("grid", ["defaults", "one_wave", "two_waves", "wave_per_window"])
def test_directory_search_behind_a_missed_guess_in_eleven_windows(engine, grid, run_optimize):
    """a.head / a.gap / a.far of the eleven-window segment: and_resolve searches three directory entries and finds the container, three
    and finds none, two to the left of the guess (tests/test_roaring_cases_cpu.py restates the arithmetic)."""
    seg = RC.segment("skip", run_optimize)
    queries = RC.skip_queries(seg)
    executed, _ = run_corpus(engine, seg, queries, "skip", GRIDS[grid])
    assert executed == len(queries) == 45


def test_batch_of_one_two_and_six_windows(engine):
    """index_and_batch_kernel: four-wave workgroups, items with fewer windows than waves.  Each index-led corpus query that all three
    sizes can name goes through one pg_execute_batch call over six segments (1, 2 and 6 windows, run-optimised and not), twice -- the
    second call meets the plan cache -- and every result equals the single execution and the model."""
    segs = [RC.segment(key, opt) for key in ("w1", "w2", "main") for opt in (True, False)]
    lists = [RC.batch_queries(s) for s in segs]
    labels = [(q.label, q.aggs) for q in lists[0] if all(any((p.label, p.aggs) == (q.label, q.aggs) for p in other) for other in lists[1:])]
    assert len(labels) >= 60
    opened = [engine.open(s.data) for s in segs]
    try:
        items = 0
        for label, aggs in labels:
            qs = [next(p for p in lst if (p.label, p.aggs) == (label, aggs)) for lst in lists]
            specs = [q.spec(s) for q, s in zip(qs, segs)]
            singles = [g.execute(spec) for g, spec in zip(opened, specs)]
            for rep in range(2):
                for i, (status, res) in enumerate(engine.execute_batch(opened, specs)):
                    assert status == _abi.PG_OK, (label, segs[i].key, rep, engine.lib.pg_last_error())
                    RC.assert_matches_model(res, RC.model(segs[i], qs[i]), qs[i], "batch %s rep %d" % (segs[i].key, rep))
                    assert answer(res) == answer(singles[i]), (label, segs[i].key, rep)
                    items += 1
        print("batch: %d items, 0 declined" % items)
    finally:
        [g.close() for g in opened]
