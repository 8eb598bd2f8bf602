"""Chunk-compressed raw forward indexes: fixtures and cases shared by test_chunk_codec_cpu.py and test_gpu_chunk_codec.py (a helper, not a test).

* write_file: the fixed-byte chunk file of BaseChunkForwardIndexWriter, versions 1 to 4, over a list of already-compressed chunks.
* lz4_compress / snappy_compress: small greedy compressors (LZ4 block format, Snappy raw format) -- a GPU machine need not have liblz4.
* Block: hand-assembled chunks for the formats' edges; it builds the compressed bytes and, beside them, the bytes they must decode to (a
  match is DEFINED here as a byte-by-byte copy from `distance` back).
* case(name): one column per shape -- the compressed file, its PASS_THROUGH twin, the values.

Every comparison is the device (or the host decoder) on the compressed file against the oracle / numpy on the same values written
PASS_THROUGH: the oracle declines compressed files and stays that way."""
import functools

import numpy as np

PASS_THROUGH, SNAPPY, ZSTANDARD, LZ4, LZ4_LENGTH_PREFIXED, GZIP = 0, 1, 2, 3, 4, 5      # ChunkCompressionType.getValue()
CODEC_NAMES = {SNAPPY: "SNAPPY", ZSTANDARD: "ZSTANDARD", LZ4: "LZ4", LZ4_LENGTH_PREFIXED: "LZ4_LENGTH_PREFIXED", GZIP: "GZIP"}
DEVICE_CHUNK_CAP = 65536      # PG_CHUNK_DECODE_MAX_BYTES: larger decoded chunks take the host decoder


# ---------------------------------------------------------------------------------------------------------------- the file
def write_file(version, codec, docs_per_chunk, entry_size, num_docs, chunks):
    """version 1: 16-byte header, 4-byte offsets, no codec field (always SNAPPY); 2: 28-byte header, 4-byte offsets; 3 and 4: 8-byte offsets."""
    be = lambda v, n=4: int(v).to_bytes(n, "big")
    head = be(version) + be(len(chunks)) + be(docs_per_chunk) + be(entry_size)
    if version > 1:
        head += be(num_docs) + be(codec) + be(28)
    else:
        assert codec == SNAPPY
    ob = 4 if version <= 2 else 8
    at = len(head) + ob * len(chunks)
    table = []
    for c in chunks:
        table.append(be(at, ob))
        at += len(c)
    return np.frombuffer(head + b"".join(table) + b"".join(bytes(c) for c in chunks), dtype=np.uint8).copy()


def big_endian_bytes(values):
    values = np.ascontiguousarray(values)
    return values.astype(values.dtype.newbyteorder(">")).tobytes()


def split_chunks(raw, chunk_bytes):
    return [raw[i:i + chunk_bytes] for i in range(0, len(raw), chunk_bytes)]


# ---------------------------------------------------------------------------------------------------------------- compressors
def _lz4_sequence(out, literals, distance, match_len):
    lit, ml = len(literals), (match_len - 4 if match_len else 0)
    out.append(min(lit, 15) << 4 | min(ml, 15))
    if lit >= 15:
        r = lit - 15
        out += b"\xff" * (r // 255) + bytes([r % 255])
    out += literals
    if match_len:
        out += bytes([distance & 255, distance >> 8])
        if ml >= 15:
            r = ml - 15
            out += b"\xff" * (r // 255) + bytes([r % 255])


def lz4_compress(data):
    """Greedy LZ4 block: a 4-byte hash table of last positions; the block's end rules are kept (the last 5 bytes are literals, no match
    starts within the last 12), so liblz4's decoder accepts it."""
    data = bytes(data)
    n, out, anchor, i, table = len(data), bytearray(), 0, 0, {}
    while i < n - 12:
        key = data[i:i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is not None and i - cand <= 65535:
            m, limit = 4, n - 5 - i
            while m < limit and data[cand + m] == data[i + m]:
                m += 1
            _lz4_sequence(out, data[anchor:i], i - cand, m)
            i += m
            anchor = i
        else:
            i += 1
    _lz4_sequence(out, data[anchor:], 0, 0)
    return bytes(out)


def _varint(n):
    out = bytearray()
    while n >= 128:
        out.append(n & 127 | 128)
        n >>= 7
    out.append(n)
    return bytes(out)


def _snappy_literal(out, literals):
    n = len(literals)
    if n == 0:
        return
    if n <= 60:
        out.append((n - 1) << 2)
    else:
        nb = 1 if n <= 256 else 2 if n <= 65536 else 3
        out.append((59 + nb) << 2)
        out += (n - 1).to_bytes(nb, "little")
    out += literals


def _snappy_copy(out, distance, length):
    while length > 0:
        n = min(length, 64)
        if 4 <= n <= 11 and distance < 2048:
            out += bytes([1 | (n - 4) << 2 | (distance >> 8) << 5, distance & 255])
        else:
            out += bytes([2 | (n - 1) << 2, distance & 255, distance >> 8])
        length -= n


def snappy_compress(data):
    """Greedy Snappy raw format: varint length, literals, copy-1 / copy-2 elements."""
    data = bytes(data)
    n, out, anchor, i, table = len(data), bytearray(_varint(len(data))), 0, 0, {}
    while i + 4 <= n:
        key = data[i:i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is not None and i - cand <= 65535:
            m = 4
            while i + m < n and data[cand + m] == data[i + m]:
                m += 1
            _snappy_literal(out, data[anchor:i])
            _snappy_copy(out, i - cand, m)
            i += m
            anchor = i
        else:
            i += 1
    _snappy_literal(out, data[anchor:])
    return bytes(out)


COMPRESSORS = {LZ4: lz4_compress, SNAPPY: snappy_compress, PASS_THROUGH: bytes}


# ---------------------------------------------------------------------------------------------------------------- hand-assembled chunks
class Block:
    """One chunk under construction.  Literal bytes are made so that the big-endian INT values they spell stay small (two zero bytes, two
    bytes below 23), which keeps sums and group counts of the edge columns modest whatever the matches shift around."""

    def __init__(self, codec, zeros=False):
        self.codec, self.z, self.raw, self.zeros = codec, bytearray(), bytearray(), zeros

    def _literals(self, n):
        p = len(self.raw)
        lit = bytes(n) if self.zeros else bytes(0 if (p + i) % 4 < 2 else ((p + i) * 7 + 3) % 23 for i in range(n))
        self.raw += lit
        return lit

    def _match(self, distance, n):
        assert 0 < distance <= len(self.raw)
        for _ in range(n):
            self.raw.append(self.raw[-distance])

    # LZ4: one sequence (match_len 0: literals only, the block's last sequence)
    def lz4(self, lit, distance=0, match_len=0):
        _lz4_sequence(self.z, self._literals(lit), distance, match_len)
        if match_len:
            self._match(distance, match_len)
        return self

    # Snappy elements; extra: force the 1..4-byte length form of the literal tag
    def literal(self, n, extra=None):
        lit = self._literals(n)
        if extra is None:
            _snappy_literal(self.z, lit)
        else:
            self.z.append((59 + extra) << 2)
            self.z += (n - 1).to_bytes(extra, "little") + lit
        return self

    def copy1(self, distance, n):
        assert 4 <= n <= 11 and distance < 2048
        self.z += bytes([1 | (n - 4) << 2 | (distance >> 8) << 5, distance & 255])
        self._match(distance, n)
        return self

    def copy2(self, distance, n):
        assert 1 <= n <= 64 and distance < 65536
        self.z += bytes([2 | (n - 1) << 2, distance & 255, distance >> 8])
        self._match(distance, n)
        return self

    def copy4(self, distance, n):
        assert 1 <= n <= 64
        self.z += bytes([3 | (n - 1) << 2]) + distance.to_bytes(4, "little")
        self._match(distance, n)
        return self

    def finish(self, target):
        """Pads with one last literal run to `target` decoded bytes (LZ4: at least the 5 literals a block must end with)."""
        rest = target - len(self.raw)
        assert rest >= (5 if self.codec == LZ4 else 0), (target, len(self.raw))
        if self.codec == LZ4:
            self.lz4(rest)
            return bytes(self.z), bytes(self.raw)
        if rest:
            self.literal(rest)
        return _varint(len(self.raw)) + bytes(self.z), bytes(self.raw)


def edge_blocks(codec, target):
    """[(name, compressed, raw)]: every edge of the format in a chunk of exactly `target` decoded bytes (target >= 5000)."""
    out = []
    add = lambda name, block: out.append((name,) + block.finish(target))
    B = lambda: Block(codec)
    if codec == LZ4:
        add("literal-only", B())
        add("empty-literal-run-before-a-match", B().lz4(4, 4, 8).lz4(0, 2, 5))
        for lit in (14, 15, 270, 271, 15 + 255 * 3):                      # token only, 15+0, 15+255+0, 15+255+1, three full length bytes
            add("literal-%d-distance-equals-produced" % lit, B().lz4(lit, lit, 4))
        for ml in (4, 18, 19, 274, 275, 1000):                           # the same for match lengths (minimum match 4)
            add("match-%d" % ml, B().lz4(40, 33, ml))
        for d in (1, 2, 3, 4, 63, 64, 65):
            add("distance-%d" % d, B().lz4(d + 2, d, 4).lz4(1, d, d + 1 if d >= 3 else 4).lz4(0, d, 64 * d + 70).lz4(3, d, 129))      # longer than the distance by 1, and by more than 64 x
        return out      # (literal-only is the incompressible chunk too: its compressed form is larger than the raw one)
    for n in (1, 59, 60, 61, 256, 257):                                  # tags 0..59, 60 (1 length byte), 61 (2 length bytes)
        add("literal-%d" % n, B().literal(n))
    add("literal-tags-62-63", B().literal(5, 3).literal(7, 4))
    for n in (4, 11):                                                    # copy-1 at its shortest and longest, offsets above 255; distance == produced
        add("copy1-%d" % n, B().literal(300).copy1(299, n).copy1(300 + n, n))
    for d in (1, 2, 3, 4, 63, 64, 65):
        blk = B().literal(d + 1).copy1(d, 5).copy2(d, 64).copy2(d, min(d + 1, 64)).copy4(d, 33)
        for _ in range(d + 2):                                           # a run longer than 64 x its distance
            blk.copy2(d, 64)
        add("distance-%d" % d, blk)
    add("copy2-copy4-far", B().literal(3000).copy2(2999, 64).copy4(3000, 1).copy4(3065, 64))
    add("incompressible", B().literal(target))
    return out


def long_match_block(codec, target):
    """1 literal, then one match at distance 1 over (almost) the whole chunk of `target` zero bytes: the longest length chain."""
    blk = Block(codec, zeros=True)
    if codec == LZ4:
        return blk.lz4(1, 1, target - 1 - 5).finish(target)
    blk.literal(1)
    while len(blk.raw) < target:
        blk.copy2(1, min(64, target - len(blk.raw)))
    return blk.finish(target)


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, version, codec, values, docs_per_chunk, chunks=None):
        self.name, self.version, self.codec, self.docs_per_chunk = name, version, codec, docs_per_chunk
        self.values = np.ascontiguousarray(values)
        self.num_docs, self.entry_size = int(self.values.shape[0]), self.values.dtype.itemsize
        raw = big_endian_bytes(self.values)
        raw_chunks = split_chunks(raw, docs_per_chunk * self.entry_size)
        self.chunks = chunks if chunks is not None else [COMPRESSORS[codec](c) for c in raw_chunks]
        self.raw_chunks = raw_chunks
        self.file = write_file(version, codec, docs_per_chunk, self.entry_size, self.num_docs, self.chunks)
        # the twin: the same header version where PASS_THROUGH can be said (version 1 cannot), the same values
        self.twin = write_file(max(version, 2), PASS_THROUGH, docs_per_chunk, self.entry_size, self.num_docs, raw_chunks)

    @property
    def chunk_bytes(self):
        return self.docs_per_chunk * self.entry_size


def _typed_values(dtype, n, seed):
    rng = np.random.default_rng(seed)
    base = np.cumsum(rng.integers(0, 3, n)).astype(np.int64)       # slowly increasing with repeats: compressible, few hundred distinct values per thousand docs
    if dtype == np.int32:
        return (base * 7 - 1000).astype(np.int32)
    if dtype == np.int64:
        return base * 1000 + 1_600_000_000_000                     # timestamps
    if dtype == np.float32:
        return (base * 0.25 - 3.0).astype(np.float32)
    return base * 0.125 + 100.2356


def _edge_case(codec, name):
    target = 5000                                                   # 1250 INT docs per chunk
    blocks = edge_blocks(codec, target)
    raw = b"".join(b[2] for b in blocks) + blocks[0][2][:4 * 7]     # ... and a last chunk of 7 docs
    tail = Block(codec).finish(4 * 7)
    assert tail[1] == blocks[0][2][:4 * 7]
    values = np.frombuffer(raw, dtype=">i4").astype(np.int32)
    return Case(name, 2, codec, values, 1250, chunks=[b[1] for b in blocks] + [tail[0]])


def _long_match_case(codec, name):
    target = 65536 - 8                                              # 8191 LONG docs: the largest chunk below the device cap that is not the cap
    z, raw = long_match_block(codec, target)
    z2, raw2 = Block(codec).finish(8 * 3)
    values = np.frombuffer(raw + raw2, dtype=">i8").astype(np.int64)
    return Case(name, 3, codec, values, 8191, chunks=[z, z2])


_SHAPES = {
    # name: (version, dtype, num_docs, docs_per_chunk)
    "one-doc": (2, np.int32, 1, 1000),
    "last-chunk-one-doc": (2, np.int64, 2001, 1000),
    "exact-multiple": (3, np.float64, 3000, 1000),
    "one-doc-per-chunk": (2, np.int32, 37, 1),
    "power2-v4": (4, np.int64, 5 * 1024 + 17, 1024),
    "float-v3": (3, np.float32, 4321, 1000),
    "double-v2": (2, np.float64, 2500, 1000),
    "int-many-chunks": (2, np.int32, 40_003, 1000),
    "cap-exact": (3, np.int64, 8192 + 5, 8192),                    # 65 536-byte chunks: the device cap itself
    "over-cap": (3, np.int64, 16384 + 1000, 16384),                # 131 072-byte chunks: the host decoder whatever the switch says
}

CASE_NAMES = (["lz4-" + s for s in _SHAPES] + ["snappy-" + s for s in _SHAPES] + ["snappy-v1-double", "snappy-v1-int"]
              + ["lz4-edges", "snappy-edges", "lz4-long-match", "snappy-long-match"])


@functools.lru_cache(maxsize=None)
def case(name):
    codec_name, shape = name.split("-", 1)
    codec = LZ4 if codec_name == "lz4" else SNAPPY
    if shape == "edges":
        return _edge_case(codec, name)
    if shape == "long-match":
        return _long_match_case(codec, name)
    if shape == "v1-double":
        return Case(name, 1, SNAPPY, _typed_values(np.float64, 3 * 700 - 5, 5), 700)
    if shape == "v1-int":
        return Case(name, 1, SNAPPY, _typed_values(np.int32, 2049, 6), 1000)
    version, dtype, n, dpc = _SHAPES[shape]
    return Case(name, version, codec, _typed_values(dtype, n, len(name)), dpc)


def golden_files():
    """The reference's own compressed files (tests/golden): (name, file bytes, num_docs, expected doubles)."""
    import base64
    import json
    import os
    out = []
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for fname in ("fixedByteCompressed_v2.json", "fixedByteSVRDoubles_v1.json"):
        g = json.load(open(os.path.join(here, fname)))
        data = np.frombuffer(base64.b64decode(g["file_base64"]), dtype=np.uint8).copy()
        out.append((fname, data, g["num_docs"], np.arange(g["num_docs"], dtype=np.float64) + g["start_value"]))
    return out
