"""CPU tests of the chunk codecs (pinot_amd/csrc/pg_chunk_codec.h): the host decoder built on the parsers the device kernel shares, against
the reference's own compressed files and the constructed corpus of tests/chunk_codec_cases.py; the segment loader; the sanitizer program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import chunk_codec_cases as CC
import segment_dirs as D
from pinot_amd import host
from pinot_amd import segment as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEND = 1      # pgcodec::kEnd: the chunk decoded to exactly the expected size


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def decode_file(file, num_docs, entry_size):
    lib = S.load_host_library()
    file = np.ascontiguousarray(file, dtype=np.uint8)
    out = np.zeros(max(num_docs * entry_size, 1), dtype=np.uint8)
    status = int(lib.ph_raw_decode_file(_u8p(file), file.nbytes, num_docs, _u8p(out)))
    return status, out[:num_docs * entry_size].tobytes()


def decode_chunk(codec, z, expect):
    lib = S.load_host_library()
    src = np.frombuffer(bytes(z) + b"\0", dtype=np.uint8).copy()      # (never empty; the size passed is the chunk's)
    out = np.zeros(max(expect, 1), dtype=np.uint8)
    return int(lib.ph_chunk_decode(codec, _u8p(src), len(z), _u8p(out), expect)), out[:expect].tobytes()


def test_the_references_compressed_files_decode_to_their_values():
    """fixedByteCompressed.v2 (SNAPPY, 2 x 1000 doubles: i + 100.2356 -- the value area of fixedByteRaw.v2, byte for byte) and
    fixedByteSVRDoubles.v1 (version 1, 3 chunks of 5003 docs, 10009 doubles: i): FixedByteChunkSVForwardIndexTest.java:344-375."""
    import base64
    import json
    (n2, f2, d2, w2), (n1, f1, d1, w1) = CC.golden_files()
    assert (f2.nbytes, d2, f1.nbytes, d1) == (8098, 2000, 44397, 10009)
    for file, docs, want in ((f2, d2, w2), (f1, d1, w1)):
        status, got = decode_file(file, docs, 8)
        assert status == 0 and np.array_equal(np.frombuffer(got, dtype=">f8").astype(np.float64), want)
    raw = base64.b64decode(json.load(open(os.path.join(ROOT, "tests", "golden", "fixedByteRaw_v2.json")))["file_base64"])
    assert decode_file(f2, d2, 8)[1] == raw[28 + 4 * 2:]
    assert int.from_bytes(f1[:4].tobytes(), "big") == 1 and int.from_bytes(f1[8:12].tobytes(), "big") == 5003


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_every_case_of_the_corpus_decodes_byte_for_byte(name):
    c = CC.case(name)
    status, got = decode_file(c.file, c.num_docs, c.entry_size)
    assert status == 0 and got == CC.big_endian_bytes(c.values)
    assert len(c.chunks) == -(-c.num_docs // c.docs_per_chunk)
    for z, raw in zip(c.chunks, c.raw_chunks):
        assert decode_chunk(c.codec, z, len(raw)) == (KEND, bytes(raw))
        assert decode_chunk(c.codec, z, len(raw) + 4)[0] != KEND and decode_chunk(c.codec, z[:-1], len(raw))[0] != KEND


def test_the_edge_corpus_holds_what_it_says():
    """Each hand-assembled chunk really is the edge its name says: the tokens are looked at, not trusted."""
    lz = {n: z for n, z, _ in CC.edge_blocks(CC.LZ4, 5000)}
    assert lz["literal-14-distance-equals-produced"][0] >> 4 == 14
    assert lz["literal-15-distance-equals-produced"][:2] == bytes([0xF0, 0]) and lz["literal-270-distance-equals-produced"][:3] == bytes([0xF0, 255, 0])
    assert lz["literal-271-distance-equals-produced"][:3] == bytes([0xF0, 255, 1])
    assert lz["empty-literal-run-before-a-match"][7] >> 4 == 0      # token, 4 literals, 2 offset bytes: the second token has no literals
    assert lz["match-18"][0] & 15 == 14 and lz["match-19"][0] & 15 == 15 and lz["match-19"][44] == 0 and lz["match-274"][44:46] == bytes([255, 0])
    assert len(lz["literal-only"]) > 5000
    sn = {n: z for n, z, _ in CC.edge_blocks(CC.SNAPPY, 5000)}
    assert sn["literal-60"][2] == 59 << 2 and sn["literal-61"][2:4] == bytes([60 << 2, 60]) and sn["literal-257"][2:5] == bytes([61 << 2, 0, 1])
    assert sn["literal-tags-62-63"][2] == 62 << 2 and sn["copy1-11"][2 + 3 + 300] == (1 | 7 << 2 | 1 << 5)
    assert len(sn["incompressible"]) > 5000
    for codec in (CC.LZ4, CC.SNAPPY):
        z, raw = CC.long_match_block(codec, 65536 - 8)
        assert len(raw) == 65528 and raw.count(0) == 65528 and decode_chunk(codec, z, 65528) == (KEND, raw)


def test_our_lz4_agrees_with_liblz4_both_ways():
    try:
        lz4 = C.CDLL("liblz4.so.1")
    except OSError:
        pytest.skip("liblz4.so.1 is not on this machine")
    lz4.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    lz4.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    lz4.LZ4_compressBound.argtypes = [C.c_int]
    for name in CC.CASE_NAMES:
        if not name.startswith("lz4-"):
            continue
        c = CC.case(name)
        for z, raw in zip(c.chunks, c.raw_chunks):
            # the Python compressor's (and the hand-assembled) blocks are LZ4 blocks to liblz4 ...
            out = C.create_string_buffer(len(raw))
            assert lz4.LZ4_decompress_safe(bytes(z), out, len(z), len(raw)) == len(raw) and out.raw == bytes(raw), name
            # ... and liblz4's blocks decode with ours
            bound = lz4.LZ4_compressBound(len(raw))
            theirs = C.create_string_buffer(bound)
            size = lz4.LZ4_compress_default(bytes(raw), theirs, len(raw), bound)
            assert size > 0 and decode_chunk(CC.LZ4, theirs.raw[:size], len(raw)) == (KEND, bytes(raw)), name


def test_the_file_checks_come_before_any_chunk():
    c = CC.case("lz4-last-chunk-one-doc")
    assert decode_file(c.file, c.num_docs, 8)[0] == 0
    assert decode_file(c.file, c.num_docs - 1, 8)[0] == 1 and "numChunks" in host._lib().ph_last_error().decode()      # 2000 docs are 2 chunks, the file has 3
    bad = c.file.copy()
    bad[28 + 4:28 + 8] = np.frombuffer((int.from_bytes(bad[28:32].tobytes(), "big") - 1).to_bytes(4, "big"), dtype=np.uint8)      # chunk 1 starts before chunk 0
    assert decode_file(bad, c.num_docs, 8)[0] == 1 and "offsets" in host._lib().ph_last_error().decode()
    bad = c.file.copy()
    bad[28 + 8:28 + 12] = np.frombuffer((c.file.nbytes + 1).to_bytes(4, "big"), dtype=np.uint8)      # chunk 2 starts past the file
    assert decode_file(bad, c.num_docs, 8)[0] == 1
    for codec in (CC.ZSTANDARD, CC.LZ4_LENGTH_PREFIXED, CC.GZIP, CC.PASS_THROUGH):
        other = c.file.copy()
        other[20:24] = np.frombuffer(codec.to_bytes(4, "big"), dtype=np.uint8)
        assert decode_file(other, c.num_docs, 8)[0] == 2
    cut = c.file[:-3].copy()
    assert decode_file(cut, c.num_docs, 8)[0] == 3 and "chunk 2" in host._lib().ph_last_error().decode()


def test_the_loader_takes_lz4_and_snappy_raw_columns_and_names_the_rest(tmp_path):
    lz, sn = CC.case("lz4-last-chunk-one-doc"), CC.case("snappy-last-chunk-one-doc")
    n = lz.num_docs
    assert sn.num_docs == n
    v1 = CC.Case("v1", 1, CC.SNAPPY, lz.values.astype(np.float64), 1000)
    zstd = lz.file.copy()
    zstd[20:24] = np.frombuffer(CC.ZSTANDARD.to_bytes(4, "big"), dtype=np.uint8)
    cols = [S.Column.raw_file("a_lz4", lz.file, np.int64), S.Column.raw_file("b_snappy", sn.file, np.int64), S.Column.raw_file("c_v1", v1.file, np.float64),
            S.Column.raw_file("d_zstd", zstd, np.int64), S.Column.raw_file("e_plain", lz.twin, np.int64), S.Column.dict_encoded("k", (np.arange(n) % 7).astype(np.int32))]
    for write in (D.write_v1, D.write_v3):
        seg = host.DirectorySegment(write(tmp_path, "compressed_" + write.__name__, n, cols), device=-1)
        try:
            d = seg.describe()
            assert [c["name"] for c in d["columns"]] == ["a_lz4", "b_snappy", "c_v1", "e_plain", "k"]
            assert len(d["notOffloaded"]) == 1 and d["notOffloaded"][0].startswith("d_zstd:") and "ZSTANDARD" in d["notOffloaded"][0]
            assert all(not c["hasDictionary"] for c in d["columns"][:4])
        finally:
            seg.destroy()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with the sanitizer runtimes")
def test_the_codec_check_is_clean_under_asan_and_ubsan():
    """host/check/chunk_codec_main.cpp: the edge corpus into exactly-sized heap buffers and every malformed chunk through the shared parsers
    (no Python in the sanitized process)."""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "pinot_amd", "csrc"), "-s", "sanitize-chunk-codec"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode("utf-8", "replace")
    assert out.returncode == 0, text[-4000:]
    assert text.strip().splitlines()[-1] == "ok" and "AddressSanitizer" not in text and "runtime error" not in text, text[-4000:]


def test_the_kernel_and_the_host_decoder_share_one_parser():
    kernel = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_chunk_decode.h")).read()
    assert '#include "pg_chunk_codec.h"' in kernel and "pgcodec::next_sequence<CODEC>(parser, s)" in kernel
    assert "src[" not in kernel.replace("src[lit_off + i]", "")      # the one read of compressed bytes outside the parser: a literal the parser returned
    engine = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_engine.hip")).read()
    assert "pgcodec::validate_chunk_table" in engine and "pgcodec::decode_file_host" in engine


def test_the_cap_is_one_number_everywhere():
    import re
    from pinot_amd import _abi
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert int(re.search(r"#define PG_CHUNK_DECODE_MAX_BYTES (\d+)", header).group(1)) == _abi.PG_CHUNK_DECODE_MAX_BYTES == CC.DEVICE_CHUNK_CAP == 65536
