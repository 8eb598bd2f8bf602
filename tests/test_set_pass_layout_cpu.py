"""CPU test: the set passes' scratch arithmetic (pinot_amd/csrc/pg_set_pass_layout.h -- what plan_distinct / plan_percentile price and the passes
allocate) under AddressSanitizer + UBSan, through its stand-alone check program (no Python in the sanitized process)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
def test_the_layout_check_is_clean_under_asan_and_ubsan():
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "pinot_amd", "csrc"), "-s", "sanitize-layout"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode("utf-8", "replace")
    assert out.returncode == 0, text[-4000:]
    assert text.strip().splitlines()[-1] == "ok" and "AddressSanitizer" not in text and "runtime error" not in text, text[-4000:]


def test_the_planners_and_the_pass_size_the_scratch_with_the_same_functions():
    engine = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_engine.hip")).read()
    assert '#include "pg_set_pass_layout.h"' in engine
    # no second copy of the arithmetic in the engine
    assert "by_width" not in engine and "slack_words(int bits" not in engine
    arm = engine[engine.index("static pg_status arm_bitsets"):engine.index("static pg_status arm_collect")]
    assert "matrices.add(counters," in arm and "hll_staged_base(matrices.total_words())" in arm and "hll_scratch_words(" in arm and "hll_staged_words(" in arm
    for begin, end, add in (("static pg_status plan_distinct", "static void distinct_agg_value", "bitsets.add(false, product,"),
                            ("static pg_status plan_percentile", "static int64_t append_count_row", "counters.add(true, product,")):
        plan = engine[engine.index(begin):engine.index(end)]
        assert add in plan and "total_words() * 4ull" in plan
    assert "hll_staged_words(product, slot.second) * 4ull" in engine
