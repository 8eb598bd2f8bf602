#!/usr/bin/env python3
"""python tools/measure_moments.py [rows] [out.json] -- VAR_POP(v) WHERE f < 100 beside SUM(v) WHERE f < 100 on bench.py's segment shape, and the same pair grouped by f (1000 groups); the two
queries of a pair alternate in one process.  Device times are the engine's HIP events around all launches of a query (pg_result.device_ms)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C
import numpy as np
import torch  # noqa: F401
import bench
from pinot_amd import _abi, query as Q, segment as S
from pinot_amd.engine import Engine

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "moments", "variance_vs_sum.json")
steps, warmup = 30, 5
engine = Engine(device_id=0, time_kernels=True)
t0 = time.time()
seg = bench.c2b_segment(S, 0, rows, "affine")
gen_s = time.time() - t0
flt = Q.leaf(Q.Pred.dict_range(1, 0, 100))
pairs = {"scalar f<100": (Q.QuerySpec([(Q.SUM, 0)], filter=flt), Q.QuerySpec([(Q.VARIANCE, 0)], filter=flt)),
         "1000 groups, no filter": (Q.QuerySpec([(Q.SUM, 0)], group_by=[1]), Q.QuerySpec([(Q.VARIANCE, 0)], group_by=[1]))}
out = {"rows": rows, "steps": steps, "warmup": warmup, "gen_s": round(gen_s, 1), "cases": {}}
with engine.open(seg) as g:
    res = _abi.pg_result()
    for name, (sum_spec, var_spec) in pairs.items():
        times = {"sum": [], "variance": []}
        walls = {"sum": [], "variance": []}
        kernels = {}
        for i in range(warmup + steps):
            for kind, spec in (("sum", sum_spec), ("variance", var_spec)):
                t = time.perf_counter()
                st = g.execute_raw(spec, res)
                w = (time.perf_counter() - t) * 1e3
                assert st == _abi.PG_OK, g.lib.pg_last_error()
                if i >= warmup:
                    times[kind].append(res.device_ms); walls[kind].append(w)
                    kernels[kind] = _abi.KERNEL_NAMES.get(int(res.dominant_kernel), "")
                g.lib.pg_result_free(C.byref(res))
        case = {}
        for kind in ("sum", "variance"):
            a = np.array(times[kind]); b = np.array(walls[kind])
            case[kind] = {"device_ms_mean": float(a.mean()), "device_ms_min": float(a.min()), "device_ms_max": float(a.max()),
                          "call_ms_host_clock_mean": float(b.mean()), "dominant_kernel": kernels[kind]}
        case["ratio_device_ms"] = case["variance"]["device_ms_mean"] / case["sum"]["device_ms_mean"]
        out["cases"][name] = case
    got = g.execute(pairs["scalar f<100"][1])
    out["scalar_tuple"] = list(got.aggregations[0].moments)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(out, open(out_path, "w"), indent=1)
print(json.dumps(out))
