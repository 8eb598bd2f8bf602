"""Randomised parity of GROUP BY over key spaces above the array-based threshold (tests/fuzz_group_cases.py): the device against the oracle
AND against the exact model, under every routing such a query can take and on two grid sizes.

Routings (ROUTINGS): the default (below 2^22 docs: the direct HBM table of group_private_kernel); PINOT_GPU_GROUP_PARTITION=force (the
partitioned path at any doc count: histogram, scatter / packed scatter, re-scatter, LDS aggregation); force with unpacked records; force
without the second level; partitioning off; partitioning and the lane-private kernel off (scan_group_kernel's HBM branch).  Each on the
whole device and with PINOT_GPU_TEST_CUS=1, where a scatter workgroup runs many rounds and the last one has idle waves.

Per generated query:
  * helpers.assert_results_equal(device, oracle, check_stats=True) and the exact model (fuzz_cases.check_result): counts, integer sums,
    MIN / MAX exactly, DOUBLE sums within count * 2^-53 * sum|x| -- through test_gpu_fuzz_typed.check_query;
  * rows in ascending raw-key order, group_id_upper_bound and num_groups_limit_reached as the oracle's, the raw keys of the rows those
    the generator computes from the key digits -- under a binding limit the first keys in docId order (group_map_cases.admitted_keys);
  * dominant_kernel: group_partition_scatter_kernel exactly when the routing forces partitioning and the generator's mirror of the
    planner says the query is partitionable (fuzz_group_cases.describe; without the second level: one-level key spaces only).
    "Partitionable" is run_group_by's own rule: a key space or a first-appearance holder that is map based, at most three
    accumulators, all of them in the INT32 domain, lane-private leaves.  Raw INT keys (through their key image) and first-appearance
    holders ARE partitioned -- the limit is applied afterwards by compact_map_groups.  Under null handling a query with nullable
    inputs runs in lanes and reports the kernel of the slowest: the kernel is asserted where every lane gives the same answer;
  * every query of the segment once more through pg_execute_batch, twice: the same results as the single executions;
  * field for field what the DEFAULT routing on the whole device returned (device_results.same_results).
Per routing: declines are PG_ERR_UNSUPPORTED with a message of fuzz_cases.DECLINE_ALLOW_LIST, at most 10 % of the queries; under the
forced routings every partition class of tests/test_fuzz_group_cases_cpu.py is reached with the scatter kernel from two segments.
The oracle's and the model's answers are computed once per seed (module cache) and shared by all parametrisations."""
import re

import pytest

import fuzz_cases as F
import fuzz_group_cases as G
from device_results import same_results
from oracle import oracle
from pinot_amd import _abi
from test_fuzz_group_cases_cpu import REQUIRED_CLASSES, expected_raw_keys, where
from test_gpu_fuzz_typed import MAX_DECLINED, check_query

pytestmark = pytest.mark.gpu

FORCE = {"PINOT_GPU_GROUP_PARTITION": "force"}
ROUTINGS = {
    "default": {},
    "force": FORCE,
    "force-unpacked": dict(FORCE, PINOT_GPU_PARTITION_PACKED="0"),
    "force-one-level": dict(FORCE, PINOT_GPU_PARTITION_TWO_LEVEL="0"),
    "partition-off": {"PINOT_GPU_GROUP_PARTITION": "0"},
    "staged": {"PINOT_GPU_GROUP_PRIVATE": "0", "PINOT_GPU_GROUP_PARTITION": "0"},
}
SWITCHES = ["PINOT_GPU_GROUP_PARTITION", "PINOT_GPU_PARTITION_PACKED", "PINOT_GPU_PARTITION_TWO_LEVEL", "PINOT_GPU_GROUP_PRIVATE", "PINOT_GPU_TEST_CUS"]
NOT_PARTITION_CLASSES = ("more than 3 accumulators", "non-INT32 input", "lds")
TWO_LEVEL_CLASSES = ("two-level packed", "two-level unpacked", "fine per coarse 2^1", "fine per coarse 2^2", "fine per coarse 2^3", "wide")

_REFERENCE = {}         # seed -> (segment, queries, oracle results, model results)
_DEFAULT = {}           # seed -> the default routing's results on the whole device (None where it declined)


def reference(seed):
    if seed not in _REFERENCE:
        seg = G.make_segment(seed)
        queries = G.make_queries(seg)
        _REFERENCE[seed] = (seg, queries, [oracle.execute(seg.data, fq.spec) for fq in queries], [F.expected(seg, fq) for fq in queries])
    return _REFERENCE[seed]


def execute_or_decline(g, fq, at):
    try:
        return g.execute(fq.spec)
    except _abi.PinotGpuError as e:
        assert e.status == _abi.PG_ERR_UNSUPPORTED, "%s: %s" % (at, e)
        assert any(re.search(p, str(e)) for p in F.DECLINE_ALLOW_LIST), "%s: declined outside the allow-list: %s" % (at, e)
        return None


def default_results(engine, seed):
    """What the default routing returns on the whole device (checked by its own parametrisation; here only the yardstick of the others)."""
    if seed not in _DEFAULT:
        seg, queries, _, _ = reference(seed)
        engine.reinit(**{k: None for k in SWITCHES})
        with engine.open(seg.data) as g:
            _DEFAULT[seed] = [execute_or_decline(g, fq, "default routing, " + where(seg, qi, fq)) for qi, fq in enumerate(queries)]
    return _DEFAULT[seed]


def expects_partition(routing, info):
    """Whether the query's dominant kernel is the scatter kernel; None where its lanes differ (null handling: the lane whose kernel ran
    longest names the kernel, and that is a measured time) or where the generator does not foretell it (fuzz_group_cases._lane_plan)."""
    if ROUTINGS[routing].get("PINOT_GPU_GROUP_PARTITION") != "force":
        return False
    if any(partitionable is None for partitionable, _ in info.lane_plans):
        return None
    lanes = {partitionable and (k == 0 or routing != "force-one-level") for partitionable, k in info.lane_plans}
    return lanes.pop() if len(lanes) == 1 else None


def run_seed_set(engine, routing, cus):
    env = dict({k: None for k in SWITCHES}, PINOT_GPU_TEST_CUS=cus, **ROUTINGS[routing])
    reached = {}
    generated = declined = 0
    for seed in G.SEEDS:
        seg, queries, wants, exps = reference(seed)
        yardstick = default_results(engine, seed)
        engine.reinit(**env)
        generated += len(queries)
        ran = []
        with engine.open(seg.data) as g:
            for qi, (fq, want, exp) in enumerate(zip(queries, wants, exps)):
                at = "%s, routing %s%s" % (where(seg, qi, fq), routing, ", one CU" if cus else "")
                got = execute_or_decline(g, fq, at)
                if got is None:
                    declined += 1
                    continue
                try:
                    check_query(seg, fq, got, want, exp)
                    assert list(got.groups) == sorted(got.groups), "rows not in ascending raw-key order"
                    assert got.group_id_upper_bound == want.group_id_upper_bound, "group_id_upper_bound %d, oracle %d" % (got.group_id_upper_bound, want.group_id_upper_bound)
                    assert got.num_groups_limit_reached == want.num_groups_limit_reached
                    assert set(got.groups) == expected_raw_keys(seg, fq, exp), "the admitted raw keys"
                    partitioned = got.dominant_kernel == G.SCATTER_KERNEL
                    expect = expects_partition(routing, fq.info)
                    assert expect is None or partitioned == expect, "partitionable %r (map_based %r, int32 inputs %r, lanes %r)" % (
                        fq.info.partitionable, fq.info.map_based, fq.info.int32_inputs, fq.info.lane_plans)
                    if yardstick[qi] is not None:
                        same_results(got, yardstick[qi], same_plan=False)
                except AssertionError as e:
                    raise AssertionError("%s [%s]: %s" % (at, got.dominant_kernel, e)) from e
                if partitioned and expect:
                    for label in fq.info.labels():
                        reached.setdefault(label, set()).add(seed)
                ran.append((qi, fq, got, want, exp))
            # the segment's queries in ONE pg_execute_batch, twice
            for rep in range(2):
                out = engine.execute_batch([g] * len(ran), [r[1].spec for r in ran]) if ran else []
                for (status, res), (qi, fq, single, want, exp) in zip(out, ran):
                    at = "%s, routing %s%s, batch pass %d" % (where(seg, qi, fq), routing, ", one CU" if cus else "", rep)
                    assert status == _abi.PG_OK, "%s: status %d" % (at, status)
                    try:
                        check_query(seg, fq, res, want, exp)
                        same_results(res, single)
                    except AssertionError as e:
                        raise AssertionError("%s [%s]: %s" % (at, res.dominant_kernel, e)) from e
    return reached, generated, declined


@pytest.mark.parametrize("cus", [None, "1"], ids=["whole-device", "one-cu"])
@pytest.mark.parametrize("routing", list(ROUTINGS))
def test_random_wide_key_group_bys(engine, routing, cus):
    try:
        reached, generated, declined = run_seed_set(engine, routing, cus)
    finally:
        engine.reinit(**{k: None for k in SWITCHES})
    print("group fuzz [%s%s]: %d queries, %d declined, partitioned classes %r" % (routing, ", one CU" if cus else "", generated, declined, {k: len(v) for k, v in sorted(reached.items())}))
    assert declined <= MAX_DECLINED * generated, "%d of %d generated queries declined" % (declined, generated)
    if ROUTINGS[routing].get("PINOT_GPU_GROUP_PARTITION") == "force":
        need = [k for k in REQUIRED_CLASSES if k not in NOT_PARTITION_CLASSES and not (routing == "force-one-level" and k in TWO_LEVEL_CLASSES)]
        missing = {k: sorted(reached.get(k, ())) for k in need if len(reached.get(k, ())) < 2}
        assert not missing, "partition classes reached by %s from fewer than two segments: %r" % (G.SCATTER_KERNEL, missing)
    else:
        assert not reached
