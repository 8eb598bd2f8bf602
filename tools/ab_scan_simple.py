"""A/B of scan_simple_kernel against scan_simple_pipe_kernel on a RESIDENT C2b segment (bench.py's: v 17-bit, f 10-bit over 1000 values):
SELECT SUM(v) WHERE f < t at a list of selectivities, PINOT_GPU_SCAN_SIMPLE_PIPE flipped between 0 (scan_simple_kernel) and 2 (the
pipelined kernel whatever the estimate) in one process -- Engine.reinit re-reads the switch, the segment stays open.  The settings
alternate within every round, so that a drift of the clocks falls on both.

  python tools/ab_scan_simple.py [--rows N] [--steps K] [--warmup W] [--rounds R] [--selectivities 1,2,3,5,7,10,25,50] [--out file.jsonl]

Every answer is held against the oracle once, on a segment of --check-rows rows with the same columns (both settings), and on the large
segment the two settings must give the same answer.  One JSON line per (round, selectivity, setting), and a last line per selectivity
with the medians and the ranges: the table kPipeMinSelectivityPct of pg_engine.hip is read from.  An answer that
differs -- from the oracle's, or between the settings -- ends the tool with a non-zero status (after the line that records it).
Two builds are compared by running the tool twice with PINOT_GPU_LIB set."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SWITCH = "PINOT_GPU_SCAN_SIMPLE_PIPE"
SETTINGS = (("simple", "0"), ("pipe", "2"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--check-rows", type=int, default=3_000_017)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--selectivities", default="1,2,3,5,7,10,25,50", help="per cent of f's 1000 dictIds")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch  # noqa: F401  (loads the ROCm runtime first)
    from bench import Timer, c2b_segment
    import helpers as H
    from oracle import oracle
    from pinot_amd import _abi
    from pinot_amd import query as Q
    from pinot_amd import segment as S
    from pinot_amd.engine import Engine

    percents = [int(x) for x in args.selectivities.split(",") if x]
    spec_of = lambda pct: Q.QuerySpec([(Q.SUM, 0)], filter=Q.leaf(Q.Pred.dict_range(1, 0, pct * 10)))
    answer = lambda r: (r.stats[0], [(a.count, a.sum_i64) for a in r.aggregations])
    engine = Engine(device_id=0, time_kernels=True)
    timer = Timer(engine.lib, _abi)
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    try:
        # ---- the answers, at reduced size: both settings against the oracle ----
        small = c2b_segment(S, 0, args.check_rows, "affine")
        exact = {}
        with engine.open(small) as g:
            for pct in percents:
                want = oracle.execute(small, spec_of(pct))
                exact[pct] = True
                for _name, value in SETTINGS:
                    engine.reinit(**{SWITCH: value})
                    try:
                        H.assert_results_equal(g.execute(spec_of(pct)), want, True)
                    except AssertionError:
                        exact[pct] = False
        emit({"check_rows": args.check_rows, "exact_vs_oracle": exact})
        del small
        if not all(exact.values()):
            sys.exit("ab_scan_simple: an answer differs from the oracle's at %s %% -- nothing timed" % [p for p in percents if not exact[p]])

        # ---- the times, on the resident segment ----
        seg = c2b_segment(S, 0, args.rows, "affine")
        nbytes = seg.columns[0].fwd.nbytes + seg.columns[1].fwd.nbytes
        samples = {}
        with engine.open(seg) as g:
            engine.reinit(**{SWITCH: "0"})
            timer.run(g, spec_of(10), 1, 48)             # the clock transient after idle (bench.py's settle launches)
            same = {}
            for rnd in range(args.rounds):
                for pct in percents:
                    for name, value in SETTINGS:
                        engine.reinit(**{SWITCH: value})
                        t = timer.run(g, spec_of(pct), args.steps, args.warmup)
                        if rnd == 0:
                            same.setdefault(pct, []).append(answer(g.execute(spec_of(pct))))
                        samples.setdefault((pct, name), []).append(t["kernel_ms"])
                        emit({"round": rnd, "selectivity_pct": pct, "setting": name, SWITCH: value, "rows": args.rows, "kernel": t["kernel"], "kernel_ms": t["kernel_ms"],
                              "all_kernels_ms": t["all_kernels_ms"], "host_clock_ms": t["step_ms_host_clock"], "TBps": nbytes / t["kernel_ms"] / 1e9})
        for pct in percents:
            a, b = samples[(pct, "simple")], samples[(pct, "pipe")]
            emit({"summary": True, "selectivity_pct": pct, "rows": args.rows, "rounds": args.rounds, "steps": args.steps,
                  "simple_ms": {"median": statistics.median(a), "min": min(a), "max": max(a)}, "pipe_ms": {"median": statistics.median(b), "min": min(b), "max": max(b)},
                  "pipe_over_simple": statistics.median(b) / statistics.median(a), "pipe_faster_in_every_round": max(b) < min(a),
                  "same_answer": same[pct][0] == same[pct][1], "exact_vs_oracle_at_check_rows": exact[pct]})
        differ = [pct for pct in percents if same[pct][0] != same[pct][1]]
        if differ:
            sys.exit("ab_scan_simple: the two settings answer differently at %s %%" % differ)
    finally:
        engine.reinit(**{SWITCH: None})


if __name__ == "__main__":
    main()
