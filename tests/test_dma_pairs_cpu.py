"""CPU test: the ring kernels' pair arithmetic (pinot_amd/csrc/pg_dma_pairs.h -- the slot and LDS bytes, which width pairs have an instance of
scan_simple_dma_pair_kernel and where in the table, the pieces and last-piece lanes of a tile's staging) under AddressSanitizer + UBSan, through
its stand-alone check program (no Python in the sanitized process)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pinot_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
def test_the_pair_check_is_clean_under_asan_and_ubsan():
    out = subprocess.run(["make", "-C", CSRC, "-s", "sanitize-dma-pairs"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode("utf-8", "replace")
    assert out.returncode == 0, text[-4000:]
    assert text.strip().splitlines()[-1] == "ok" and "AddressSanitizer" not in text and "runtime error" not in text, text[-4000:]


def test_the_launcher_and_the_planner_read_the_pairs_from_the_one_header():
    engine = open(os.path.join(CSRC, "pg_engine.hip")).read()
    unit = open(os.path.join(CSRC, "pg_unit_scan_simple_dma.hip")).read()
    part = open(os.path.join(CSRC, "pg_scan_simple_dma_pair_part.h")).read()
    kernel = open(os.path.join(CSRC, "pg_scan_simple_dma.h")).read()
    assert '#include "pg_dma_pairs.h"' in engine and '#include "pg_dma_pairs.h"' in kernel
    # no second copy of the rule's figures or of the slot arithmetic
    assert "kDmaMinSlotBytes = " not in engine and "kDmaBlocksPerCu = " not in engine and "dma_slot_bytes(int" not in kernel and "dma_lds_bytes(int" not in kernel
    plan = engine[engine.index("static void plan_scan_simple_dma"):engine.index("static ScanChoice choose_scan_kernel")]
    assert "dma_slot_bytes(filter_bits, value_bits)" in plan and "scan_simple_dma_pair_shape(filter_bits, value_bits)" in plan
    assert "dma_pair_index(filter_bits, value_bits) >= 0" in unit and "dma_pair_index(p.nodes[0].bits, p.agg_cols[0].bits)" in unit
    assert "dma_pair_at(" in part and "make_index_sequence<kPartPairs>" in part      # the instances come from the table, not from a list
