"""A/B of scan_simple_kernel, scan_simple_pipe_kernel and scan_simple_dma_kernel on a RESIDENT C2b segment (bench.py's: v 17-bit, f 10-bit
over 1000 values): SELECT SUM(v) WHERE f < t at a list of selectivities, the switches flipped in one process -- `simple`
(PINOT_GPU_SCAN_SIMPLE_PIPE=0, PINOT_GPU_SCAN_SIMPLE_DMA=0), `pipe` (the pipelined kernel whatever the estimate), `dma` (the LDS-ring
kernel's generic form whatever the rule says, PINOT_GPU_SCAN_SIMPLE_DMA_PAIR=0; --dma-configs adds other launches of it: `blocks_per_cu[:nt]`,
e.g. 1,2:0,2:1) and `pair` (the ring kernel's instance for the two widths, scan_simple_dma_pair_kernel; --settings dma,pair).  Engine.reinit
re-reads the switches, the segment stays open.  The settings alternate within every round, so that a drift of the clocks falls on all.

  python tools/ab_scan_simple.py [--rows N] [--steps K] [--warmup W] [--rounds R] [--selectivities 1,2,3,5,7,10,25,50] [--settings simple,pipe,dma]
                                 [--dma-configs 1,2:0] [--out file.jsonl]

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

PIPE, DMA, BPC, NT = "PINOT_GPU_SCAN_SIMPLE_PIPE", "PINOT_GPU_SCAN_SIMPLE_DMA", "PINOT_GPU_SCAN_SIMPLE_DMA_BLOCKS_PER_CU", "PINOT_GPU_SCAN_SIMPLE_DMA_NT"
PAIR = "PINOT_GPU_SCAN_SIMPLE_DMA_PAIR"
UNSET = {PIPE: None, DMA: None, BPC: None, NT: None, PAIR: None}
# `dma`: the ring kernel's generic form (scan_simple_dma_kernel<N, aux>); `pair`: its form with both widths compile-time constants
# (scan_simple_dma_pair_kernel<10, 17, aux> here), which is what the switch at 2 alone launches for this segment
BASE_SETTINGS = {"simple": dict(UNSET, **{PIPE: "0", DMA: "0"}), "pipe": dict(UNSET, **{PIPE: "2", DMA: "0"}), "dma": dict(UNSET, **{DMA: "2", PAIR: "0"}),
                 "pair": dict(UNSET, **{DMA: "2"})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--check-rows", type=int, default=3_000_017)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--selectivities", default="1,2,3,5,7,10,25,50", help="per cent of f's 1000 dictIds")
    ap.add_argument("--settings", default="simple,pipe,dma")
    ap.add_argument("--dma-configs", default="", help="further launches of the ring kernel, blocks_per_cu[:nt], comma separated")
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
    SETTINGS = [(name, BASE_SETTINGS[name]) for name in args.settings.split(",") if name]
    for cfg in [c for c in args.dma_configs.split(",") if c]:
        parts = cfg.split(":")
        SETTINGS.append(("dma-b%s%s" % (parts[0], "-nt" + parts[1] if len(parts) > 1 else ""), dict(UNSET, **{DMA: "2", PAIR: "0", BPC: parts[0], NT: parts[1] if len(parts) > 1 else None})))
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
                    engine.reinit(**value)
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
            engine.reinit(**BASE_SETTINGS["simple"])
            timer.run(g, spec_of(10), 1, 48)             # the clock transient after idle (bench.py's settle launches)
            same = {}
            for rnd in range(args.rounds):
                for pct in percents:
                    for name, value in SETTINGS:
                        engine.reinit(**value)
                        t = timer.run(g, spec_of(pct), args.steps, args.warmup)
                        if rnd == 0:
                            same.setdefault(pct, []).append(answer(g.execute(spec_of(pct))))
                        samples.setdefault((pct, name), []).append(t["kernel_ms"])
                        emit({"round": rnd, "selectivity_pct": pct, "setting": name, "rows": args.rows, "kernel": t["kernel"], "kernel_ms": t["kernel_ms"],
                              "all_kernels_ms": t["all_kernels_ms"], "host_clock_ms": t["step_ms_host_clock"], "TBps": nbytes / t["kernel_ms"] / 1e9})
        names = [name for name, _ in SETTINGS]
        for pct in percents:
            stats = {name: {"median": statistics.median(samples[(pct, name)]), "min": min(samples[(pct, name)]), "max": max(samples[(pct, name)])} for name in names}
            emit({"summary": True, "selectivity_pct": pct, "rows": args.rows, "rounds": args.rounds, "steps": args.steps, "kernel_ms": stats,
                  "over_first": {name: stats[name]["median"] / stats[names[0]]["median"] for name in names[1:]},
                  "fastest_in_every_round": [name for name in names if all(stats[name]["max"] < stats[o]["min"] for o in names if o != name)],
                  "same_answer": all(a == same[pct][0] for a in same[pct]), "exact_vs_oracle_at_check_rows": exact[pct]})
        differ = [pct for pct in percents if any(a != same[pct][0] for a in same[pct])]
        if differ:
            sys.exit("ab_scan_simple: the settings answer differently at %s %%" % differ)
    finally:
        engine.reinit(**UNSET)


if __name__ == "__main__":
    main()
