"""GPU tests of scan_simple_pipe_kernel (pinot_amd/csrc/pg_scan_simple_pipe.h): scan_simple_kernel's shape with one dictionary-range
leaf AND one aggregated packed column, the two columns' loads software-pipelined across a wave's tiles (v(i) and f(i+1) are requested
before f(i) is decoded).  Every case runs three ways -- PINOT_GPU_SCAN_SIMPLE_PIPE=2 (the pipelined kernel whenever the shape allows),
=0 (scan_simple_kernel) and the oracle -- and all three are bit equal; both kernels report `scan_simple_kernel`.

The shapes are the smallest at which a pipeline can go wrong: zero, one, two and three or more tiles per wave (a prologue without a
loop, a peeled last tile), every class of sixteen-byte loads per column, segments that end on a tile boundary (the last lanes' last
load starts early so that it ends with the tile), and the masks at their edges."""
import csv
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from pinot_amd import query as Q
from pinot_amd import segment as S
import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALL_FUNCTIONS = [(Q.COUNT, -1), (Q.MIN, 1), (Q.MAX, 1), (Q.AVG, 1)]


def answer(res):
    return res.stats[0], [(a.count, a.sum_i64, a.min, a.max) for a in res.aggregations]


@pytest.fixture
def three_ways(engine):
    def run(seg, specs, cus=None):
        """Every spec on one open segment: the pipelined kernel, scan_simple_kernel, the oracle.  cus: PINOT_GPU_TEST_CUS (read when the segment opens)."""
        had = os.environ.get("PINOT_GPU_TEST_CUS")
        if cus is not None:
            os.environ["PINOT_GPU_TEST_CUS"] = str(cus)
        try:
            with engine.open(seg) as g:
                for spec in specs:
                    want = oracle.execute(seg, spec)
                    got = {}
                    for mode in ("2", "0"):
                        engine.reinit(PINOT_GPU_SCAN_SIMPLE_PIPE=mode)
                        got[mode] = g.execute(spec)
                        assert got[mode].dominant_kernel == "scan_simple_kernel", (mode, got[mode].dominant_kernel)
                        H.assert_results_equal(got[mode], want, True)
                    assert answer(got["2"]) == answer(got["0"])
        finally:
            engine.reinit(PINOT_GPU_SCAN_SIMPLE_PIPE=None)
            if cus is not None:
                if had is None:
                    os.environ.pop("PINOT_GPU_TEST_CUS", None)
                else:
                    os.environ["PINOT_GPU_TEST_CUS"] = had
    return run


def headline_columns(n, seed):
    """f: 10 bits (1000 values), v: 17 bits (100 000 values, affine: the dictId stream is its own value plane) -- the headline's widths."""
    f = S.Column.synthetic_uniform("f", n, np.arange(1000, dtype=np.int32), seed=seed)
    v = S.Column.synthetic_uniform("v", n, (np.arange(100000, dtype=np.int64) * 7 + 3).astype(np.int32), seed=seed + 1)
    assert f.bits == 10 and v.bits == 17
    return f, v


def headline_specs():
    return [Q.QuerySpec([(Q.SUM, 1)], filter=Q.leaf(Q.Pred.dict_range(0, 0, 100))),
            Q.QuerySpec(ALL_FUNCTIONS, filter=Q.leaf(Q.Pred.dict_range(0, 300, 800)))]


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 40960, 43009, 100003])
def test_tiles_per_wave_on_one_compute_unit(three_ways, n):
    """Grids sized for one CU: 20 resident waves, and lean_grid launches 8 of them for up to 40 tiles.  One or two tiles for 8 waves (waves
    without a tile, waves whose only iteration is their last), 20 tiles = one per resident wave and 22 (two or three per launched wave),
    49 tiles for 20 waves (100 003 docs)."""
    f, v = headline_columns(n, 10 + n % 97)
    three_ways(S.SegmentData("t%d" % n, n, [f, v]), headline_specs(), cus=1)


def test_most_waves_without_a_tile_on_the_full_grid(three_ways):
    f, v = headline_columns(70001, 5)
    three_ways(S.SegmentData("full", 70001, [f, v]), headline_specs())


@pytest.mark.parametrize("fbits,vbits", [(1, 20), (4, 17), (5, 16), (8, 13), (9, 12), (10, 17), (12, 9), (13, 8), (16, 5), (16, 16),
                                          (17, 8), (17, 10), (20, 1), (20, 20)])
def test_width_classes_across_the_sixteen_byte_load_boundaries(three_ways, fbits, vbits):
    """Both sides of every boundary between N and N + 1 sixteen-byte loads per lane, as the filter and as the aggregated column; ragged sizes,
    affine dictionaries.  One-bit columns are the width at which three lanes (61 to 63), not one, start their last load early.  (16, 16)
    and (17, 8) are the widest pairs with an instantiation, <4, 4> and <5, 2>.  (17, 10) and (20, 20) have none -- <5, 3> and <5, 5> spill
    at five waves per SIMD -- and stay with scan_simple_kernel under either setting."""
    n = 6151 + 37 * fbits
    cf = 2 ** fbits - (1 if fbits > 1 and fbits % 3 == 0 else 0)
    cv = 2 ** vbits - (1 if vbits > 1 and vbits % 2 == 0 else 0)
    f = S.Column.synthetic_uniform("f", n, np.arange(cf, dtype=np.int32) * 2 - 9, seed=fbits)
    v = S.Column.synthetic_uniform("v", n, (np.arange(cv, dtype=np.int64) * 7 + 3).astype(np.int32), seed=100 + vbits)
    assert f.bits == fbits and v.bits == vbits
    lo, hi = cf // 4, max(cf // 4 + 1, (3 * cf) // 4)
    three_ways(S.SegmentData("w%d_%d" % (fbits, vbits), n, [f, v]),
               [Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, 1), (Q.MIN, 1), (Q.MAX, 1), (Q.AVG, 1)], filter=Q.leaf(Q.Pred.dict_range(0, lo, hi))),
                Q.QuerySpec([(Q.SUM, 1)], filter=Q.leaf(Q.Pred.dict_range(0, 0, max(1, cf // 3)))),
                Q.QuerySpec([(Q.COUNT, -1), (Q.MAX, 1)], filter=Q.leaf(Q.Pred.dict_range(0, lo, hi, exclusive=True)))], cus=1)


@pytest.mark.parametrize("tiles", [1, 2, 21, 45])
def test_segments_that_end_on_a_tile_boundary(three_ways, tiles):
    """n = 2048 k: the last lane of the last tile owns real docs, and its last sixteen-byte load (20 dwords for a 17-bit column's 17, 12 for
    a 10-bit column's 10) starts three or two dwords early, ends with the column's last tile, and is moved up in registers."""
    n = 2048 * tiles
    f, v = headline_columns(n, 40 + tiles)
    three_ways(S.SegmentData("b%d" % tiles, n, [f, v]), headline_specs(), cus=1)


def test_masks_at_their_edges(three_ways):
    n = 3 * 2048 + 777
    rng = np.random.default_rng(11)
    ids = rng.integers(0, 500, n).astype(np.int32)             # dictIds 500 .. 999 exist in the dictionary and in no doc ...
    ids[n - 1] = 777                                           # ... but for the last doc of the last tile
    f = S.Column.from_dict_ids("f", np.arange(1000, dtype=np.int32) * 3 - 50, ids)
    v = S.Column.synthetic_uniform("v", n, (np.arange(100000, dtype=np.int64) * 7 + 3).astype(np.int32), seed=3)
    seg = S.SegmentData("masks", n, [f, v])
    leaf = lambda lo, hi, **kw: Q.leaf(Q.Pred.dict_range(0, lo, hi, **kw))
    specs = []
    for aggs in ([(Q.SUM, 1)], ALL_FUNCTIONS):
        specs += [Q.QuerySpec(aggs, filter=leaf(600, 700)),                    # no doc matches
                  Q.QuerySpec(aggs, filter=leaf(0, 999)),                      # every doc matches
                  Q.QuerySpec(aggs, filter=leaf(777, 778)),                    # one match: the last doc of the last tile
                  Q.QuerySpec(aggs, filter=leaf(123, 345)),                    # lo != 0
                  Q.QuerySpec(aggs, filter=leaf(100, 400, exclusive=True)),    # an exclusive range
                  Q.QuerySpec(aggs, filter=leaf(0, 778, exclusive=True))]      # ... that excludes every doc
    three_ways(seg, specs, cus=1)
    with_match = oracle.execute(seg, specs[2])
    assert with_match.aggregations[0].count == 1


PROBE = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch  # noqa: F401
from pinot_amd import query as Q
from pinot_amd import segment as S
from pinot_amd.engine import Engine
n = 100003
f = S.Column.synthetic_uniform("f", n, np.arange(1000, dtype=np.int32), seed=2)
v = S.Column.synthetic_uniform("v", n, (np.arange(100000, dtype=np.int64) * 7 + 3).astype(np.int32), seed=1)
seg = S.SegmentData("rule", n, [f, v])
engine = Engine(device_id=0, time_kernels=False)
with engine.open(seg) as g:
    for t in %(thresholds)r:
        r = g.execute(Q.QuerySpec([(Q.SUM, 1)], filter=Q.leaf(Q.Pred.dict_range(0, 0, t))))
        assert r.dominant_kernel == "scan_simple_kernel", r.dominant_kernel
    for mode, t in (("2", 10), ("0", 100)):
        engine.reinit(PINOT_GPU_SCAN_SIMPLE_PIPE=mode)
        r = g.execute(Q.QuerySpec([(Q.SUM, 1)], filter=Q.leaf(Q.Pred.dict_range(0, 0, t))))
        assert r.dominant_kernel == "scan_simple_kernel", r.dominant_kernel
print("probe ok")
"""


def test_the_rule_sends_selective_filters_to_scan_simple_kernel(tmp_path):
    """The default switch, a 1000-value filter dictionary: f < 100 (10 %) and f < 500 (50 %) run the pipelined kernel, f < 10 (1 %) runs
    scan_simple_kernel -- kPipeMinSelectivityPct of pg_engine.hip lies between.  Then the switch as the other tests of this file set it:
    at 2 the 1 % filter runs the pipelined kernel, at 0 the 10 % filter runs scan_simple_kernel (both report one name: only the trace
    tells them apart).  One rocprofv3 --kernel-trace run, the launches in order."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(rocprof), "rocprofv3 is part of the image"
    out_dir = str(tmp_path / "trace")
    env = dict(os.environ, TMPDIR="/tmp")
    for k in list(env):
        if k.startswith("PINOT_GPU_") and k not in ("PINOT_GPU_LIB",):
            del env[k]
    script = tmp_path / "probe.py"
    script.write_text(PROBE % {"root": ROOT, "thresholds": [100, 500, 10]})
    proc = subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", out_dir, "-o", "rule", "--", sys.executable, str(script)],
                          cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert proc.returncode == 0 and b"probe ok" in proc.stdout, proc.stderr.decode()[-3000:]
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as fh:
            rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh) if "scan_simple" in r["Kernel_Name"]]
    names = [name for _, name in sorted(rows)]
    assert len(names) == 5, names
    assert "scan_simple_pipe_kernel<3, 5>" in names[0] and "scan_simple_pipe_kernel<3, 5>" in names[1], names
    assert "scan_simple_kernel" in names[2] and "pipe" not in names[2], names
    assert "scan_simple_pipe_kernel<3, 5>" in names[3], names
    assert "scan_simple_kernel" in names[4] and "pipe" not in names[4], names
