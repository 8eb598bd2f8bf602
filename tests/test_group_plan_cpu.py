"""CPU test: the group-by plan's arithmetic (pinot_amd/csrc/pg_group_plan.h -- the partition plan, the packing rules, pass B's chunk and the
partitioned path's buffer layout) under AddressSanitizer + UBSan, through its stand-alone check program (no Python in the sanitized process);
and the Python mirror of that arithmetic (tests/fuzz_group_cases.py `plan` and its constants) against what the program prints."""
import os
import shutil
import subprocess

import pytest

import fuzz_group_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCTS = [10001, 4096 * 512 - 1, 4096 * 512, 4096 * 512 + 1, 2048 * 512 - 1, 2048 * 512, 2048 * 512 + 1, 1 << 21, 1 << 22, 1 << 23,
            (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 31) - 1]


@pytest.fixture(scope="module")
def check_output():
    if shutil.which("g++") is None:
        pytest.skip("needs g++ with the sanitizer runtimes")
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "pinot_amd", "csrc"), "-s", "sanitize-group-plan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode("utf-8", "replace")
    assert out.returncode == 0, text[-4000:]
    return text


def _fields(line):
    words = line.split()
    return {words[i]: int(words[i + 1]) for i in range(1, len(words), 2)}


def test_the_plan_check_is_clean_under_asan_and_ubsan(check_output):
    text = check_output
    assert text.strip().splitlines()[-1] == "ok" and "AddressSanitizer" not in text and "runtime error" not in text, text[-4000:]


def test_the_python_mirror_plans_what_the_engine_header_plans(check_output):
    lines = check_output.splitlines()
    limits = [_fields(l) for l in lines if l.startswith("limits ")]
    assert len(limits) == 1
    assert limits[0]["max_partitions"] == G.MAX_PARTITIONS and limits[0]["max_partition_aggs"] == G.MAX_PARTITION_AGGS
    assert limits[0]["max_fine_per_coarse"] == G.MAX_FINE_PER_COARSE and limits[0]["repartition_chunk"] == G.REPARTITION_CHUNK
    plans = [_fields(l) for l in lines if l.startswith("plan ")]
    # (4096 * 512 is 2^21: the list names that product twice, and so does the program)
    assert [(f["product"], f["accumulators"]) for f in plans] == [(p, a) for p in PRODUCTS for a in range(4)]
    for f in plans:
        product, accumulators = f["product"], f["accumulators"]
        assert f["entry_bytes"] == 4 + 8 * accumulators
        assert (f["shift"], f["fine"], f["log2_fine_per_coarse"], f["scatter"]) == G.plan(product, accumulators), (product, accumulators)


def test_the_engine_plans_with_the_header_and_keeps_no_second_copy():
    engine = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_engine.hip")).read()
    assert '#include "pg_group_plan.h"' in engine
    # no second copy of the arithmetic in the engine: the shift rule, the level count, the layout's offsets, the packing rules, the chunk
    assert "? 12 : 11" not in engine and "entry_bytes <= 20" not in engine and "4 + 8 * gp.num_group_aggs" not in engine
    assert "size_t off_" not in engine and "align(N * 4)" not in engine and "want_chunk" not in engine
    assert "2 * cbits" not in engine and "unsigned_field" not in engine
    route = engine[engine.index("static pg_status choose_group_route"):engine.index("static pg_status size_group_launch")]
    assert "partition_plan(p->product, gp.num_group_aggs, kMaxPartitions)" in route and "partition_packed_bits(g_engine.partition_packed," in route
    size = engine[engine.index("static pg_status size_group_launch"):engine.index("static pg_status init_group_table")]
    assert "count_bits(docs_per_block)" in size and "count_packed_shift(cbits, ga.bits)" in size
    part = engine[engine.index("static pg_status run_partitioned_group_by"):engine.index("struct PresentGroups")]
    assert "const PartitionLayout lay(" in part and "sizeof(PartitionWork), kRepartitionChunk)" in part and "partition_chunk(total_upper, seg->num_cus," in part
    # the default of numGroupsLimit is spelled once
    assert engine.count("num_groups_limit > 0") == 1
