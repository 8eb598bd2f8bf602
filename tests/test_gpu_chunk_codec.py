"""LZ4- and Snappy-compressed raw columns on the device: pg_segment_open decodes the chunks (chunk_decode_kernel, pg_chunk_decode.h) and the
column is its PASS_THROUGH twin from then on.

The oracle declines compressed files and stays that way: every comparison is the device on the COMPRESSED file against the oracle (or the
numpy HyperLogLog model) on the same values written PASS_THROUGH -- the twin.  Integer results are bit exact; SUM over FLOAT / DOUBLE
values is helpers.FP_SUM_RTOL as everywhere.  On a library without the feature every open here answers PG_ERR_UNSUPPORTED."""
import numpy as np
import pytest

import chunk_codec_cases as CC
import helpers as H
import hll_cases as HL
from oracle import oracle
from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S

pytestmark = pytest.mark.gpu

R, K, V = 0, 1, 2      # the raw column under test, a small dictionary key, a dictionary value column


def segments(c):
    """(segment over the compressed file, segment over its PASS_THROUGH twin): the raw column plus two dictionary columns."""
    rng = np.random.default_rng(c.num_docs)
    k = S.Column.dict_encoded("k", rng.integers(0, 9, c.num_docs).astype(np.int32))
    v = S.Column.dict_encoded("v", rng.integers(-500, 500, c.num_docs).astype(np.int32))
    dtype = c.values.dtype
    return (S.SegmentData("z_" + c.name, c.num_docs, [S.Column.raw_file("r", c.file, dtype), k, v]),
            S.SegmentData("t_" + c.name, c.num_docs, [S.Column.raw_file("r", c.twin, dtype), k, v]))


def value_window(values):
    """(lo, hi, members): a run of at most 200 consecutive DISTINCT values of the column around its median -- as an IN list it matches
    exactly the docs the range [lo, hi] matches, which is how the oracle (it has no IN on raw columns) answers the same query."""
    u = np.unique(values)
    a = max(0, len(u) // 2 - 100)
    members = u[a:a + 200]
    return members[0], members[-1], members


def queries(c):
    """[(id, device spec, oracle spec | None)] -- one query of each consumer family of a raw column."""
    lo, hi, members = value_window(c.values)
    floating = np.issubdtype(c.values.dtype, np.floating)
    rng_leaf = Q.leaf(Q.Pred.raw_range_f64(R, float(lo), float(hi)) if floating else Q.Pred.raw_range(R, int(lo), int(hi)))
    in_leaf = Q.leaf(Q.Pred.raw_set_f64(R, [float(m) for m in members]) if floating else Q.Pred.raw_set(R, [int(m) for m in members]))
    range_sum = Q.QuerySpec([(Q.SUM, R), (Q.COUNT, -1), (Q.MIN, R), (Q.MAX, R)], filter=rng_leaf)
    raw_in = Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, V)], filter=in_leaf)
    raw_in_oracle = Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, V)], filter=rng_leaf)
    group = Q.QuerySpec([(Q.SUM, V), (Q.COUNT, -1)], filter=rng_leaf, group_by=[R])
    return [("range-sum", range_sum, range_sum), ("in", raw_in, raw_in_oracle), ("group-by-raw-key", group, group),
            ("hll", Q.QuerySpec([(Q.hll(), R), (Q.COUNT, -1)], filter=Q.leaf(Q.Pred.dict_range(K, 0, 5))), None)]


def read_all(g, c):
    docs = np.arange(c.num_docs, dtype=np.int32)
    if c.values.dtype == np.int32:
        return g.read_int_values(R, docs)
    if c.values.dtype == np.int64:
        return g.read_long_values(R, docs)
    return g.read_double_values(R, docs)


def check_case(engine, c, expect_same_bytes=True):
    zseg, tseg = segments(c)
    HL.set_values(tseg, R, c.values)
    with engine.open(zseg) as g, engine.open(tseg) as t:
        got = read_all(g, c)
        want = c.values.astype(np.float64) if np.issubdtype(c.values.dtype, np.floating) else c.values
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), "values differ"      # bit equal
        if expect_same_bytes:
            assert g.device_bytes() == t.device_bytes()
        for qid, spec, oracle_spec in queries(c):
            twin = t.execute(spec)
            for rep in range(2):
                r = g.execute(spec)
                where = "%s %s run %d" % (c.name, qid, rep)
                assert r.dominant_kernel == twin.dominant_kernel, where
                if oracle_spec is not None:
                    H.assert_results_equal(r, oracle.execute(tseg, oracle_spec))
                else:
                    HL.assert_registers_equal(r, tseg, spec, where=where)
                    H.assert_agg_equal(r.aggregations[1], oracle.execute(tseg, HL.without_hll(spec)).aggregations[1], Q.COUNT, where)


def test_the_references_compressed_files_open_as_they_are(engine):
    """fixedByteCompressed.v2 (SNAPPY) and fixedByteSVRDoubles.v1 (version 1), written by the reference: FixedByteChunkSVForwardIndexTest.java:344-375."""
    for name, data, n, want in CC.golden_files():
        seg = S.SegmentData(name, n, [S.Column.raw_file("d", data, np.float64)])
        twin = S.SegmentData(name + "_twin", n, [S.Column.raw_typed("d", want)])
        with engine.open(seg) as g:
            assert np.array_equal(g.read_double_values(0, np.arange(n, dtype=np.int32)), want)
            spec = Q.QuerySpec([(Q.COUNT, -1), (Q.SUM, 0), (Q.MIN, 0), (Q.MAX, 0)])
            r = g.execute(spec)
            H.assert_results_equal(r, oracle.execute(twin, spec))
            assert r.aggregations[0].count == n and r.aggregations[2].min == want[0] and r.aggregations[3].max == want[-1]


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_a_compressed_column_is_its_pass_through_twin(engine, name):
    c = CC.case(name)
    check_case(engine, c, expect_same_bytes=c.version != 1)      # (a version-1 header is 12 bytes shorter than any PASS_THROUGH file's: no twin of the same layout)


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_the_host_decoder_gives_the_same_column(engine, name):
    """PINOT_GPU_CHUNK_DECODE=host: the chunks are decoded by the host decoder and uploaded as values; the over-cap shape takes that path with the switch unset."""
    c = CC.case(name)
    engine.reinit(PINOT_GPU_CHUNK_DECODE="host")
    try:
        check_case(engine, c, expect_same_bytes=c.version != 1)
    finally:
        engine.reinit(PINOT_GPU_CHUNK_DECODE=None)


def test_the_cap_is_where_the_cases_say():
    assert CC.case("lz4-cap-exact").chunk_bytes == CC.DEVICE_CHUNK_CAP == _abi.PG_CHUNK_DECODE_MAX_BYTES
    assert CC.case("lz4-over-cap").chunk_bytes == 2 * CC.DEVICE_CHUNK_CAP and CC.case("lz4-long-match").chunk_bytes == CC.DEVICE_CHUNK_CAP - 8


def _open_status(engine, file, num_docs, dtype=np.int64):
    seg = S.SegmentData("declined", num_docs, [S.Column.raw_file("r", file, dtype)])
    with pytest.raises(_abi.PinotGpuError) as ei:
        engine.open(seg).close()
    return ei.value.status, str(ei.value)


def test_what_is_still_declined(engine):
    c = CC.case("lz4-last-chunk-one-doc")
    for codec in (CC.ZSTANDARD, CC.LZ4_LENGTH_PREFIXED, CC.GZIP):
        other = c.file.copy()
        other[20:24] = np.frombuffer(codec.to_bytes(4, "big"), dtype=np.uint8)
        status, text = _open_status(engine, other, c.num_docs)
        assert status == _abi.PG_ERR_UNSUPPORTED and CC.CODEC_NAMES[codec] in text and "compressionType=%d" % codec in text
    # the offset table is checked on the host, before any launch: decreasing offsets, an offset past the file, a chunk count that does not fit numDocs
    bad = c.file.copy()
    bad[28 + 4:28 + 8] = np.frombuffer((int.from_bytes(bad[28:32].tobytes(), "big") - 1).to_bytes(4, "big"), dtype=np.uint8)
    status, text = _open_status(engine, bad, c.num_docs)
    assert status == _abi.PG_ERR_INVALID_ARGUMENT and "offsets" in text
    bad = c.file.copy()
    bad[28 + 8:28 + 12] = np.frombuffer((c.file.nbytes + 1).to_bytes(4, "big"), dtype=np.uint8)
    status, text = _open_status(engine, bad, c.num_docs)
    assert status == _abi.PG_ERR_INVALID_ARGUMENT and "offsets" in text
    status, text = _open_status(engine, c.file, c.num_docs - 1)
    assert status == _abi.PG_ERR_INVALID_ARGUMENT and "numChunks" in text
    status, text = _open_status(engine, c.file, c.num_docs, dtype=np.int32)      # sizeOfEntry 8 for an INT column
    assert status == _abi.PG_ERR_UNSUPPORTED and "entry size" in text


def test_compressed_and_plain_segments_in_one_batch(engine):
    """pg_execute_batch over segments of which some hold the compressed column and some the twin: the items are equal pairwise."""
    cases = [CC.case("lz4-int-many-chunks"), CC.case("snappy-int-many-chunks"), CC.case("lz4-edges"), CC.case("snappy-v1-int")]
    segs = [s for c in cases for s in segments(c)]
    opened = [engine.open(s) for s in segs]
    try:
        for make in (lambda c: queries(c)[0][1], lambda c: Q.QuerySpec([(Q.COUNT, -1)], filter=Q.leaf(Q.Pred.raw_range(R, int(value_window(c.values)[0]), int(value_window(c.values)[1]))))):
            specs = [make(c) for c in cases for _ in range(2)]
            for rep in range(2):
                results = engine.execute_batch(opened, specs)
                assert all(status == _abi.PG_OK for status, _ in results)
                for i, c in enumerate(cases):
                    z, t = results[2 * i][1], results[2 * i + 1][1]
                    H.assert_results_equal(z, t)
                    H.assert_results_equal(z, oracle.execute(segs[2 * i + 1], specs[2 * i]))
                    assert z.dominant_kernel == t.dominant_kernel
    finally:
        [g.close() for g in opened]
