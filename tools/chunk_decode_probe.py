#!/usr/bin/env python3
"""pg_segment_open of one LZ4-compressed raw LONG column of slowly increasing timestamps (1 000 docs per chunk), three ways: the chunks decoded on
the device (chunk_decode_kernel), on the host (PINOT_GPU_CHUNK_DECODE=host), and the PASS_THROUGH twin that needs no decoding.

    python tools/chunk_decode_probe.py [--docs 100000000] [--reps 5] [--modes device,host,twin]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/chunk_decode_probe.py --modes device --reps 3      (the kernel's own time)

Wall clock around pg_segment_open (it returns after the decode has finished and the compressed copy is freed), the modes alternating; one
JSON line.  The chunks are compressed with liblz4 when the machine has it (LZ4_compress_default, what the reference's LZ4Compressor calls
through lz4-java), otherwise with the Python compressor of tests/chunk_codec_cases.py over a pool of 64 chunk contents that repeat."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", default="device,host,twin")
    args = ap.parse_args()
    import chunk_codec_cases as CC
    from pinot_amd import query as Q
    from pinot_amd import segment as S
    from pinot_amd.engine import Engine

    n, dpc = args.docs, 1000
    rng = np.random.default_rng(1)
    try:
        lz4 = C.CDLL("liblz4.so.1")
        lz4.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        values = 1_600_000_000_000 + np.cumsum(rng.integers(0, 40, n, dtype=np.int64))      # milliseconds, ~20 ms apart
        raw = CC.big_endian_bytes(values)
        out = C.create_string_buffer(dpc * 8 + 64)
        chunks = []
        for at in range(0, len(raw), dpc * 8):
            piece = raw[at:at + dpc * 8]
            size = lz4.LZ4_compress_default(piece, out, len(piece), len(out))
            chunks.append(out.raw[:size])
        compressor = "liblz4"
    except OSError:
        pool = 1_600_000_000_000 + np.cumsum(rng.integers(0, 40, 64 * dpc, dtype=np.int64))
        values = np.tile(pool, n // len(pool) + 1)[:n]
        raw = CC.big_endian_bytes(values)
        packed, chunks = {}, []
        for at in range(0, len(raw), dpc * 8):
            piece = raw[at:at + dpc * 8]
            if piece not in packed:
                packed[piece] = CC.lz4_compress(piece)
            chunks.append(packed[piece])
        compressor = "python, 64 chunk contents"
    file = CC.write_file(3, CC.LZ4, dpc, 8, n, chunks)
    twin = CC.write_file(3, CC.PASS_THROUGH, dpc, 8, n, CC.split_chunks(raw, dpc * 8))
    del raw, chunks
    segs = {"device": S.SegmentData("lz4", n, [S.Column.raw_file("t", file, np.int64)]), "host": S.SegmentData("lz4", n, [S.Column.raw_file("t", file, np.int64)]),
            "twin": S.SegmentData("twin", n, [S.Column.raw_file("t", twin, np.int64)])}
    engine = Engine(device_id=0, time_kernels=False)
    spec = Q.QuerySpec([(Q.SUM, 0), (Q.COUNT, -1)])
    want = float(values.astype(np.float64).sum())
    modes = [m for m in args.modes.split(",") if m]
    times = {m: [] for m in modes}
    for rep in range(args.reps + 1):                       # (the first round is the warm-up: code objects, the staging pool)
        for m in modes:
            engine.reinit(PINOT_GPU_CHUNK_DECODE="host" if m == "host" else None)
            t0 = time.perf_counter()
            g = engine.open(segs[m])
            dt = time.perf_counter() - t0
            r = g.execute(spec)
            assert r.aggregations[1].count == n and abs(r.aggregations[0].sum - want) <= 1e-9 * abs(want), (m, r.aggregations[0].sum, want)
            g.close()
            if rep:
                times[m].append(round(dt * 1e3, 2))
    engine.reinit(PINOT_GPU_CHUNK_DECODE=None)
    print(json.dumps({"docs": n, "docs_per_chunk": dpc, "compressor": compressor, "compressed_bytes": int(file.nbytes), "twin_bytes": int(twin.nbytes),
                      "open_ms": times, "median_open_ms": {m: float(np.median(v)) for m, v in times.items() if v}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
