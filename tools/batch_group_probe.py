"""pg_execute_batch over group-bys whose rows are converted by the shared launch's closure (defer_group_item, pg_engine.hip): every kind of
holder value group_agg_value produces there -- COUNT, SUM, MIN, MAX and AVG over a plane-encoded dictionary column (affine dictionary: the
sum is scale x field sum + docs x base) and over a plain one (an irregular dictionary, gathered) -- once keyed by a dictionary column and once
by a raw INT column through its key image (numGroupsLimit at its default, above the 1000 keys).  Run by tests/test_gpu_batch.py with
PINOT_GPU_BATCH_TRACE=1 (the library says on stderr how many items every shared launch carried); every answer is held against the oracle and
against pg_execute, twice (the second call through the plan cache).  One JSON line on stdout."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

DOCS, GROUPS = 5000, 1000


def main():
    import helpers as H
    from oracle import oracle
    from pinot_amd import _abi
    from pinot_amd import query as Q
    from pinot_amd import segment as S
    from pinot_amd.engine import Engine

    engine = Engine(device_id=0)
    segs = []
    for s in range(3):
        rng = np.random.default_rng(8800 + s)
        keys = rng.integers(0, GROUPS, DOCS).astype(np.int32)
        keys[rng.permutation(DOCS)[:GROUPS]] = np.arange(GROUPS, dtype=np.int32)           # every key present: the raw column spans exactly GROUPS values
        kd = S.Column.from_dict_ids("kd", (np.arange(GROUPS, dtype=np.int64) * 3 - 17).astype(np.int32), keys)
        kr = S.Column.raw("kr", (keys.astype(np.int64) - 500 + s).astype(np.int32))
        # plane-encoded: base -100000 - s (not zero: the docs x base term), scale 7; MIN / MAX fold its dictIds
        p = S.Column.synthetic_uniform("p", DOCS, (np.arange(300, dtype=np.int64) * 7 - 100000 - s).astype(np.int32), seed=31 * s + 1)
        # plain: 300 sorted distinct values from the whole int32 range, both ends present
        pool = np.unique(np.concatenate([rng.integers(-2 ** 31, 2 ** 31, 298), [-2 ** 31, 2 ** 31 - 1]])).astype(np.int32)
        q = S.Column.synthetic_uniform("q", DOCS, pool, seed=31 * s + 2)
        segs.append(S.SegmentData("bg%d" % s, DOCS, [kd, kr, p, q]))
    aggs = [(Q.COUNT, -1)] + [(f, c) for c in (2, 3) for f in (Q.SUM, Q.MIN, Q.MAX, Q.AVG)]
    shapes = {"dictionary-key": lambda s: Q.QuerySpec(aggs, group_by=[0]),
              "raw-int-key": lambda s: Q.QuerySpec(aggs, group_by=[1]),
              "raw-int-key-filtered": lambda s: Q.QuerySpec(aggs, filter=Q.leaf(Q.Pred.dict_range(2, 10 + s, 200)), group_by=[1])}
    report = {"failed": [], "shapes": {}}
    opened = [engine.open(seg) for seg in segs]
    try:
        for name, make in shapes.items():
            specs = [make(s) for s in range(len(segs))]
            wants = [oracle.execute(seg, spec) for seg, spec in zip(segs, specs)]
            sys.stderr.write("== shape %s\n" % name)
            sys.stderr.flush()
            for rep in range(2):
                for s, (status, res) in enumerate(engine.execute_batch(opened, specs)):
                    try:
                        assert status == _abi.PG_OK
                        H.assert_results_equal(res, wants[s])
                        assert res.group_keys == wants[s].group_keys and res.group_id_upper_bound == wants[s].group_id_upper_bound
                        assert res.num_groups_limit_reached == wants[s].num_groups_limit_reached
                        if rep == 0:
                            single = opened[s].execute(specs[s])
                            H.assert_results_equal(single, wants[s])
                            assert res.stats == single.stats and res.group_keys == single.group_keys and res.group_id_upper_bound == single.group_id_upper_bound
                    except AssertionError as e:
                        report["failed"].append([name, rep, s, str(e)[:200]])
            report["shapes"][name] = len(segs)
    finally:
        [g.close() for g in opened]
    print(json.dumps(report))


if __name__ == "__main__":
    main()
