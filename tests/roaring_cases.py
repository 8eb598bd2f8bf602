"""A constructed corpus of RoaringBitmap container edges for the three device paths that decode serialized bitmaps -- index_and_kernel /
index_and_batch_kernel (pinot_amd/csrc/pg_index_and.h), roaring_expand_kernel (pg_kernels.h) and parse_roaring (pg_engine.hip).

Nothing is random.  A RECIPE says which window-relative docs a NAMED dictId of a column owns in which 65 536-doc window; every doc left
over belongs to the column's filler, dictId 0, whose posting (the complement) is part of the corpus.  A recipe is cut to the segment:
windows the segment does not have and docs past its end drop out, a name that is left without a doc gets no dictId in that segment, and
the queries that mention it are not generated for it.  Names, not dictIds, are what the queries are written in.

census(column) reads the index bytes with a reader written from the public RoaringFormatSpec (independent of parse_roaring and of the
oracle's reader); model(segment, query) answers a query with numpy from the dictId arrays alone.  Every figure is an integer: all
comparisons are exact.  Nothing here needs a GPU or the oracle."""
import struct

import numpy as np

from pinot_amd import query as Q
from pinot_amd import segment as S

W = 65536
# name -> numDocs.  main: six windows, the last one ragged (2112 docs: no multiple of 64 or of a 2048-doc tile, but 66 * 32, so the tail
# mask meets a word that must be kept whole); even: ends on a window boundary (no tail mask); one: the last window holds one doc;
# w1 / w2: the batch's one- and two-window items.
# skip: eleven windows -- the fewest at which the directory search behind a missed guess runs over three entries (SKIP_QUERIES only).
SEGMENTS = {"main": 5 * W + 2049 + 63, "even": 6 * W, "one": 2 * W + 1, "w1": W - 5, "w2": W + 4097, "skip": 10 * W + 100}
SINGLE = ("main", "even", "one")

A, B, R, G, V, F, NR, NA = range(8)               # column indexes
COLUMN_NAMES = ["a", "b", "r", "g", "v", "f", "nr", "na"]


def stride(start, step, count):
    return start + step * np.arange(count, dtype=np.int64)


def span(first, last):
    return np.arange(first, last + 1, dtype=np.int64)


def runs(start, count, length, period):
    return (start + period * np.arange(count, dtype=np.int64)[:, None] + np.arange(length, dtype=np.int64)[None, :]).ravel()


def residue(r):
    return np.arange(r, W, 8, dtype=np.int64)


def cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])


# ---- column a: the array cardinalities (and 4097, the smallest bitset) ----
# The large ones start at doc 1000 of their window, the small ones at 40 930 -- 30 docs before the 1 KB piece boundary at 40 960, so
# that a handful of docs straddles two pieces of whatever bitset they meet; stride 7 keeps every one of them an array (no runs).
def _a(card, small):
    return stride(40930 if small else 1000, 7, card)


RECIPE_A = [
    ("a4095", {0: _a(4095, False)}), ("a1", {0: _a(1, True)}),
    ("a4096", {1: _a(4096, False)}), ("a7", {1: _a(7, True)}),
    ("a4097", {2: _a(4097, False)}), ("a8", {2: _a(8, True)}),
    ("a512", {3: _a(512, False)}), ("a9", {3: _a(9, True)}),
    ("a513", {4: _a(513, False)}), ("a511", {4: _a(511, True)}),
    # the remaining lengths of an array's last 16-byte piece: with the cardinalities above (1, 7 and 8 docs in it) and atail (3), every
    # `left` of and_scatter8_some from 1 to 8
    ("a10", {0: stride(46000, 7, 10)}), ("a12", {1: stride(46000, 7, 12)}), ("a13", {2: stride(46000, 7, 13)}), ("a14", {3: stride(46000, 7, 14)}),
    # postings that skip windows so that the interpolated guess lands on another key (the third and fourth only in the skip segment,
    # where `head` is searched over three entries and found, `gap` over three and not found, `far` over two to the left of the guess)
    ("head", {w: stride(50000, 3, 201) for w in (0, 1, 2, 3, 4)}),
    ("gap", {w: stride(52000, 3, 201) for w in (0, 1, 2, 3, 5)}),
    ("far", {1: stride(54000, 3, 201), 8: stride(54000, 3, 201), 10: stride(3, 3, 31)}),
    # the column's last posting ends in an array of three docs (six bytes: the index buffer ends inside a lane's 16-byte load); in the
    # main segment doc 2111 is the segment's last
    ("atail", {5: np.array([5, 2049, 2111])}),
]

# ---- column b: window presence patterns; every eighth doc of a window = 8192 docs, a bitset (an array of 264 in main's last window) ----
RECIPE_B = [
    ("every", {w: residue(1) for w in range(6)}),
    ("first", {0: residue(0)}),
    ("last", {5: residue(0)}),
    ("firstlast", {0: residue(2), 5: residue(2)}),
    ("high", {w: residue(4) for w in (3, 4, 5)}),            # the interpolated guess is low
    ("low", {w: residue(6) for w in (0, 1, 2)}),             # ... clamps high
    ("evens", {w: residue(3) for w in (0, 2, 4)}),
    ("odds", {w: residue(3) for w in (1, 3, 5)}),
    ("uneven", {w: residue(5) for w in (0, 1, 5)}),
    ("late", {w: residue(7) for w in (0, 3, 4, 5)}),
]

# ---- column r: run containers (run_optimize=True; arrays and bitsets of the same docs otherwise) ----
RECIPE_R = [
    # three runs: one from doc 0, one of length 1, one to doc 65 535
    ("edges", {0: cat(span(0, 3000), [5000], span(60000, 65535))}),
    # 65 runs: the second trip of a wavefront's loop over the runs (130 in window 3: the third); 2047 runs of 3 docs: the most the
    # writer still stores as runs (2 + 4 * 2047 = 8190 < 8192)
    ("r65", {1: runs(0, 65, 100, 200), 3: runs(53000, 130, 20, 40)}),
    ("r2047", {1: runs(16384, 2047, 3, 4)}),
    # one window holds an array, a bitset and a run container of three dictIds: a 3-value IN child mixes the three scatter paths
    ("arr3", {3: stride(0, 16, 1000)}),
    ("bit3", {3: stride(16384, 2, 8192)}),
    ("run3", {3: cat(span(40000, 50000), span(52000, 52010))}),
    # another kind, or nothing, in every window: array, bitset, 70 runs, array, nothing, one run
    ("mix", {0: stride(20000, 5, 300), 1: stride(30000, 2, 5000), 2: runs(1000, 70, 300, 500), 3: stride(60000, 3, 100), 5: span(1100, 1500)}),
    ("full", {4: span(0, W - 1)}),                            # one run [0, 65535]; a bitset of 65 536 when not run-optimised
    ("rtail", {5: cat(span(0, 1000), span(2000, 2111))}),    # a run that ends on main's last doc
]

RECIPES = {A: RECIPE_A, B: RECIPE_B, R: RECIPE_R}
G_CARD = 64


class Segment:
    """One corpus segment in one build (run_optimize): dictId arrays, name -> dictId maps, the S.SegmentData."""

    def __init__(self, key, run_optimize):
        self.key, self.run_optimize = key, bool(run_optimize)
        n = self.n = SEGMENTS[key]
        self.windows = (n + W - 1) // W
        doc = np.arange(n, dtype=np.int64)
        self.ids = {}
        self.names = {}
        for col, recipe in RECIPES.items():
            ids = np.zeros(n, dtype=np.int32)
            names = {"filler": 0}
            for name, per_window in recipe:
                docs = cat(*[w * W + d for w, d in per_window.items()]) if per_window else np.zeros(0, np.int64)
                docs = docs[docs < n]
                if docs.shape[0] == 0:
                    continue
                assert (ids[docs] == 0).all(), "recipes of column %s overlap at %s" % (COLUMN_NAMES[col], name)
                names[name] = len(names)
                ids[docs] = names[name]
            assert (ids == 0).any()
            self.ids[col], self.names[col] = ids, names
        self.ids[G] = ((doc // 37) % G_CARD).astype(np.int32)           # 64 values, runs of 37 docs: ~28 runs per posting and window
        self.names[G] = {str(d): d for d in range(G_CARD)}
        self.ids[V] = ((doc * 40503 + 17) % 100000).astype(np.int32)
        self.ids[F] = ((doc * 7919 + 3) % 1000).astype(np.int32)
        self.ids[NR] = (doc % 2).astype(np.int32)
        self.ids[NA] = (doc % 3 == 0).astype(np.int32)
        self.dict_values = {A: np.arange(len(self.names[A]), dtype=np.int32) * 5 - 7, B: np.arange(len(self.names[B]), dtype=np.int32) * 3 + 1,
                            R: np.arange(len(self.names[R]), dtype=np.int32) * 2 - 3, G: np.arange(G_CARD, dtype=np.int32) * 11 - 100,
                            V: (np.arange(100000, dtype=np.int64) * 7 + 3).astype(np.int32),      # affine, 17 bits
                            F: np.arange(1000, dtype=np.int32) * 3 + 1,                           # 10 bits
                            NR: np.array([0, 1], dtype=np.int32), NA: np.array([0, 1], dtype=np.int32)}
        # the null vectors: postings of column r (runs from doc 0, to the window's end, a whole window, 2047 runs) and of column a
        # (every array edge, the 4097-doc bitset) as ONE serialized bitmap each -- roaring_expand_kernel's input at segment open
        self.nulls = {NR: np.isin(self.ids[R], [self.names[R][x] for x in ("edges", "r65", "r2047", "full", "rtail") if x in self.names[R]]),
                      NA: self.ids[A] != 0}
        cols = []
        for c in range(8):
            column = S.Column.from_dict_ids(COLUMN_NAMES[c], self.dict_values[c], self.ids[c], with_inverted=c in (A, B, R, G), run_optimize=self.run_optimize)
            if c in self.nulls:
                column.with_nulls(self.nulls[c])
            cols.append(column)
        assert cols[V].bits == 17 and cols[F].bits == 10
        self.data = S.SegmentData("roaring_%s_%d" % (key, int(self.run_optimize)), n, cols)

    def has(self, col, name):
        return name in self.names[col]

    def dict_id(self, col, name):
        return self.names[col][name]

    def values(self, col):
        return self.dict_values[col][self.ids[col]].astype(np.int64)


_SEGMENTS = {}


def segment(key, run_optimize):
    k = (key, bool(run_optimize))
    if k not in _SEGMENTS:
        _SEGMENTS[k] = Segment(key, run_optimize)
    return _SEGMENTS[k]


# ================================================================================================================================
# census: a reader of the inverted-index bytes from the public RoaringFormatSpec
# ================================================================================================================================
ARRAY, BITSET, RUN = "array", "bitset", "run"


def parse_bitmap(buf, start, length):
    """One serialized RoaringBitmap at buf[start : start + length] -> [(key, kind, cardinality, runs, payload offset in buf, docs)]."""
    if length == 0:
        return []
    b = bytes(buf[start:start + length])
    cookie, = struct.unpack_from("<I", b, 0)
    if cookie & 0xFFFF == 12347:
        n = (cookie >> 16) + 1
        flags = b[4:4 + (n + 7) // 8]
        is_run = [bool((flags[i >> 3] >> (i & 7)) & 1) for i in range(n)]
        pos = 4 + (n + 7) // 8
        has_offsets = n >= 4
    else:
        assert cookie == 12346, cookie
        n, = struct.unpack_from("<I", b, 4)
        is_run = [False] * n
        pos = 8
        has_offsets = True
    heads = [struct.unpack_from("<HH", b, pos + 4 * i) for i in range(n)]
    pos += 4 * n
    offsets = None
    if has_offsets:
        offsets = [struct.unpack_from("<I", b, pos + 4 * i)[0] for i in range(n)]
        pos += 4 * n
    out = []
    for i, (key, card_m1) in enumerate(heads):
        card = card_m1 + 1
        if offsets is not None:
            assert offsets[i] == pos, "offset header disagrees with the payload order"
        if is_run[i]:
            nr, = struct.unpack_from("<H", b, pos)
            pairs = np.frombuffer(b, dtype="<u2", count=2 * nr, offset=pos + 2).astype(np.int64).reshape(nr, 2)
            docs = np.concatenate([np.arange(s, s + l + 1) for s, l in pairs]) if nr else np.zeros(0, np.int64)
            out.append((key, RUN, card, nr, start + pos, docs))
            pos += 2 + 4 * nr
        elif card > 4096:
            bits = np.unpackbits(np.frombuffer(b, dtype=np.uint8, count=8192, offset=pos), bitorder="little")
            out.append((key, BITSET, card, 0, start + pos, np.flatnonzero(bits).astype(np.int64)))
            pos += 8192
        else:
            out.append((key, ARRAY, card, 0, start + pos, np.frombuffer(b, dtype="<u2", count=card, offset=pos).astype(np.int64)))
            pos += 2 * card
        assert out[-1][5].shape[0] == card
    assert pos == length, (pos, length)
    return out


def bitmap_docs(buf):
    """The docIds of one serialized RoaringBitmap (np.uint8 bytes)."""
    parts = [(key << 16) + docs for key, _, _, _, _, docs in parse_bitmap(buf, 0, len(buf))]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def posting_slices(column):
    """BitmapInvertedIndexWriter's layout: (cardinality + 1) big-endian offsets, then one serialized bitmap per dictId."""
    inv = column.inverted
    offs = np.frombuffer(bytes(inv[:4 * (column.cardinality + 1)]), dtype=">u4").astype(np.int64)
    assert offs[0] == 4 * (column.cardinality + 1) and offs[-1] == len(inv)
    return [(int(offs[d]), int(offs[d + 1] - offs[d])) for d in range(column.cardinality)]


def census(column):
    """[(dictId, key, kind, cardinality, runs, lead)]: lead = the payload's byte offset & 3 for arrays and bitsets, (offset + 2) & 3 --
    where the (start, length - 1) pairs begin -- for run containers, offsets counted from the start of the column's index buffer."""
    rows = []
    for d, (start, length) in enumerate(posting_slices(column)):
        for key, kind, card, nr, off, _ in parse_bitmap(column.inverted, start, length):
            rows.append((d, key, kind, card, nr, ((off + 2) & 3) if kind == RUN else (off & 3)))
    return rows


def posting_docs(column, d):
    start, length = posting_slices(column)[d]
    return bitmap_docs(column.inverted[start:start + length])


# ================================================================================================================================
# filters, as small tuples over NAMES; to_spec() lowers one for a segment, mask() is its numpy model
# ================================================================================================================================
def eq(col, name): return ("eq", col, name, False)
def ne(col, name): return ("eq", col, name, True)
def in_(col, names): return ("in", col, tuple(names), False)
def nin(col, names): return ("in", col, tuple(names), True)
def grange(lo, hi, exclusive=False): return ("in", G, tuple(str(d) for d in range(lo, hi)), exclusive)
def ds(col, name, exclusive=False): return ("ds", col, name, exclusive)
def null(col, exclusive=False): return ("null", col, exclusive)
def and_(*ch): return ("and",) + ch
def or_(*ch): return ("or",) + ch
def not_(ch): return ("not", ch)


def leaves(f):
    if f[0] in ("and", "or", "not"):
        for ch in f[1:]:
            for x in leaves(ch):
                yield x
    else:
        yield f


def available(seg, f):
    for lf in leaves(f):
        if lf[0] in ("eq", "ds") and not seg.has(lf[1], lf[2]):
            return False
        if lf[0] == "in" and not all(seg.has(lf[1], x) for x in lf[2]):
            return False
    return True


def mask(seg, f):
    k = f[0]
    if k in ("eq", "ds"):
        m = seg.ids[f[1]] == seg.dict_id(f[1], f[2])
        return ~m if f[3] else m
    if k == "in":
        m = np.isin(seg.ids[f[1]], [seg.dict_id(f[1], x) for x in f[2]])
        return ~m if f[3] else m
    if k == "null":
        return ~seg.nulls[f[1]] if f[2] else seg.nulls[f[1]]
    if k == "not":
        return ~mask(seg, f[1])
    parts = [mask(seg, ch) for ch in f[1:]]
    out = parts[0].copy()
    for p in parts[1:]:
        out = (out & p) if k == "and" else (out | p)
    return out


def to_spec_filter(seg, f, doc_set_ids=None):
    """The Q.Node tree.  doc_set_ids: {(col, name): id} of doc sets created on the device; None = the oracle's form, where a doc set
    is the inverted leaf of the posting it was made from (the same operator class, priority and statistics: tests/doc_set_cases.py)."""
    k = f[0]
    if k == "eq" or (k == "ds" and doc_set_ids is None):
        d = seg.dict_id(f[1], f[2])
        return Q.leaf(Q.Pred.dict_range(f[1], d, d + 1, exclusive=f[3], inverted=True))
    if k == "ds":
        return Q.leaf(Q.Pred.doc_set(doc_set_ids[(f[1], f[2])], exclusive=f[3]))
    if k == "in":
        members = sorted(seg.dict_id(f[1], x) for x in f[2])
        if members == list(range(members[0], members[-1] + 1)) and len(members) > 3:
            return Q.leaf(Q.Pred.dict_range(f[1], members[0], members[-1] + 1, exclusive=f[3], inverted=True))
        return Q.leaf(Q.Pred.dict_set(f[1], members, len(seg.names[f[1]]), exclusive=f[3], inverted=True))
    if k == "null":
        return Q.leaf(Q.Pred.is_null(f[1], exclusive=f[2]))
    if k == "not":
        return Q.not_(to_spec_filter(seg, f[1], doc_set_ids))
    return (Q.and_ if k == "and" else Q.or_)(*[to_spec_filter(seg, ch, doc_set_ids) for ch in f[1:]])


COUNT_ONLY = [(Q.COUNT, -1)]
SUM_V = [(Q.SUM, V)]
FIVE_V = [(Q.COUNT, -1), (Q.SUM, V), (Q.MIN, V), (Q.MAX, V), (Q.AVG, V)]
THREE_COLUMNS = [(Q.SUM, V), (Q.MAX, F), (Q.MIN, B)]
AGG_LISTS = [SUM_V, FIVE_V, THREE_COLUMNS]


class Query:
    def __init__(self, label, flt, aggs, group_by=()):
        self.label, self.flt, self.aggs, self.group_by = label, flt, list(aggs), list(group_by)
        kinds = {lf[0] for lf in leaves(flt)}
        self.null_handling = "null" in kinds
        self.doc_sets = sorted({(lf[1], lf[2]) for lf in leaves(flt) if lf[0] == "ds"})
        # led by the inverted indexes alone: a leaf, or an AND of leaves, every one an EQ / IN posting lookup
        self.index_led = (flt[0] in ("eq", "in")) or (flt[0] == "and" and all(ch[0] in ("eq", "in") for ch in flt[1:]))

    def spec(self, seg, doc_set_ids=None):
        return Q.QuerySpec(self.aggs, filter=to_spec_filter(seg, self.flt, doc_set_ids), group_by=self.group_by, null_handling=self.null_handling)

    def bitmap_spec(self, seg, doc_set_ids=None):
        return Q.QuerySpec([], filter=to_spec_filter(seg, self.flt, doc_set_ids), null_handling=self.null_handling)

    def certainly_gathered(self, seg):
        """The planner gathers inside index_and_kernel when its estimate -- never above the smallest inclusive child's posting -- is at
        most four docs per window: a whole-filter index AND with an inclusive EQ child of at most four docs, aggregating at most two
        columns without GROUP BY, is gathered whatever the other children hold."""
        if not self.index_led or self.group_by or len({c for _, c in self.aggs if c >= 0}) not in (1, 2):
            return False
        kids = self.flt[1:] if self.flt[0] == "and" else (self.flt,)
        return any(ch[0] == "eq" and not ch[3] and int((seg.ids[ch[1]] == seg.dict_id(ch[1], ch[2])).sum()) <= 4 for ch in kids)


def filters():
    """(label, filter) of the corpus, over names; the same list for every segment (available() drops what a segment cannot name)."""
    out = []
    add = lambda label, f: out.append((label, f))
    a_names = [name for name, _ in RECIPE_A]
    b_names = [name for name, _ in RECIPE_B]
    r_names = [name for name, _ in RECIPE_R]
    # every array edge cardinality (and the 4097-doc bitset) against a bitset posting of every window; the small ones sit across a
    # 1 KB piece boundary of it: the probe of and_single_bitset keeps one or two pieces
    for x in a_names:
        add("a.%s & b.every" % x, and_(eq(A, x), eq(B, "every")))
        add("a.%s & b.firstlast" % x, and_(eq(A, x), eq(B, "firstlast")))
    add("a.a513 & b.every & g.5", and_(eq(A, "a513"), eq(B, "every"), eq(G, "5")))
    add("a.a4096 & b.every & r.r2047", and_(eq(A, "a4096"), eq(B, "every"), eq(R, "r2047")))
    add("a.a4097 & b.low & g.40", and_(eq(A, "a4097"), eq(B, "low"), eq(G, "40")))
    # run shapes against arrays: some pairs leave a handful, some nothing in a window both are present in
    for r, a in (("edges", "a4095"), ("edges", "a1"), ("r65", "a4096"), ("r2047", "a4096"), ("r2047", "a7"), ("r65", "a512"), ("r65", "a9"),
                 ("full", "a513"), ("full", "a511"), ("rtail", "atail"), ("run3", "a9"), ("run3", "a512"), ("mix", "a4097"), ("mix", "a4095"),
                 ("arr3", "a512"), ("bit3", "a512")):
        add("r.%s & a.%s" % (r, a), and_(eq(R, r), eq(A, a)))
    for r in r_names:
        add("r.%s & b.every" % r, and_(eq(R, r), eq(B, "every")))
        add("r.%s & g.3" % r, and_(eq(R, r), eq(G, "3")))
    # every presence pattern against postings of every window (run containers of g, the bitsets of a's filler)
    for p in b_names:
        add("b.%s & g.5" % p, and_(eq(B, p), eq(G, "5")))
        add("b.%s & a.filler" % p, and_(eq(B, p), eq(A, "filler")))
        add("b.%s & r.filler & g.63" % p, and_(eq(B, p), eq(R, "filler"), eq(G, "63")))
    # IN children: 2 (array + bitset; two bitsets), 3 (array + bitset + run in one window), 16 -- all inline
    add("r IN (arr3, bit3) & b.every", and_(in_(R, ["arr3", "bit3"]), eq(B, "every")))
    add("b IN (every, low) & a.a4095", and_(in_(B, ["every", "low"]), eq(A, "a4095")))
    add("b IN (high, late) & a.filler", and_(in_(B, ["high", "late"]), eq(A, "filler")))
    add("b IN (first, last) & g.9", and_(in_(B, ["first", "last"]), eq(G, "9")))
    add("r IN (arr3, bit3, run3) & b.every", and_(in_(R, ["arr3", "bit3", "run3"]), eq(B, "every")))
    add("r IN (arr3, bit3, run3)", in_(R, ["arr3", "bit3", "run3"]))
    add("r IN (edges, mix, full) & b.odds", and_(in_(R, ["edges", "mix", "full"]), eq(B, "odds")))
    add("a IN (a4096, a7) & b IN (every, uneven)", and_(in_(A, ["a4096", "a7"]), in_(B, ["every", "uneven"])))
    # (r's filler and a4097 are the IN-member bitsets that sit at odd byte leads behind a run-flagged posting)
    add("r IN (filler, arr3) & b.every", and_(in_(R, ["filler", "arr3"]), eq(B, "every")))
    add("r IN (filler, run3, mix) & g.5", and_(in_(R, ["filler", "run3", "mix"]), eq(G, "5")))
    add("a IN (a4097, a8) & b.low", and_(in_(A, ["a4097", "a8"]), eq(B, "low")))
    add("g IN 16 & b.every", and_(grange(0, 16), eq(B, "every")))
    add("g IN 16 scattered & a.filler", and_(in_(G, [str(d) for d in range(1, 64, 4)]), eq(A, "filler")))
    add("g IN 16", grange(20, 36))
    # children that go dense before the AND: 17 postings; more than 64 postings in all (4 x 16 inline, the fifth child dense)
    add("g IN 17 & b.every", and_(grange(3, 20), eq(B, "every")))
    add("g IN 17 & r.full", and_(grange(40, 57), eq(R, "full")))
    add("65 postings", and_(grange(0, 16), grange(8, 24), grange(12, 28), grange(14, 30), eq(B, "every")))
    add("66 postings, b IN 2 dense", and_(grange(0, 16), grange(8, 24), grange(12, 28), grange(14, 30), in_(B, ["every", "low"])))
    # exclusive members: absent from some windows, the whole window, the last window's tail, NOT IN, alone
    add("b != high & g.7", and_(ne(B, "high"), eq(G, "7")))
    add("b != low & a.a513", and_(ne(B, "low"), eq(A, "a513")))
    add("r != full & g.7", and_(ne(R, "full"), eq(G, "7")))
    add("r != full & b.every", and_(ne(R, "full"), eq(B, "every")))
    add("r != full & a.a513", and_(ne(R, "full"), eq(A, "a513")))             # everything in a513's only window is excluded
    add("r != rtail & b.last", and_(ne(R, "rtail"), eq(B, "last")))
    add("a != atail & r.rtail", and_(ne(A, "atail"), eq(R, "rtail")))
    add("r NOT IN (arr3, bit3, run3) & b.every", and_(nin(R, ["arr3", "bit3", "run3"]), eq(B, "every")))
    add("b NOT IN (every, firstlast) & a.filler", and_(nin(B, ["every", "firstlast"]), eq(A, "filler")))
    add("b != every & r != full", and_(ne(B, "every"), ne(R, "full")))
    add("g NOT IN 17 & b.every", and_(grange(3, 20, exclusive=True), eq(B, "every")))
    add("r NOT IN (edges, full)", nin(R, ["edges", "full"]))
    add("g NOT IN 16", grange(0, 16, exclusive=True))
    # every named posting on its own, plain and flipped: every container of the corpus at whatever lead it has, as the only child
    for col, names in ((A, a_names), (B, b_names), (R, r_names)):
        for x in ["filler"] + names:
            add("%s.%s" % (COLUMN_NAMES[col], x), eq(col, x))
            add("%s != %s" % (COLUMN_NAMES[col], x), ne(col, x))
    for d in ("0", "31", "63"):
        add("g.%s" % d, eq(G, d))
        add("g != %s" % d, ne(G, d))
    # the same postings through roaring_expand_kernel: inverted leaves under OR and NOT ...
    for col, names in ((A, a_names), (R, r_names)):
        for x in names:
            add("%s.%s | g.63" % (COLUMN_NAMES[col], x), or_(eq(col, x), eq(G, "63")))
    for x in r_names + ["filler"]:
        add("NOT r.%s" % x, not_(eq(R, x)))
    for x in ("every", "last", "uneven"):
        add("NOT b.%s" % x, not_(eq(B, x)))
    add("NOT (r IN 3 | a.a4097)", not_(or_(in_(R, ["arr3", "bit3", "run3"]), eq(A, "a4097"))))
    add("(r.edges | r.rtail | a.atail) & b != every", and_(or_(eq(R, "edges"), eq(R, "rtail"), eq(A, "atail")), ne(B, "every")))
    # ... as doc sets made of a posting's docs, plain and flipped, alone and behind the index AND ...
    for col, x in [(R, x) for x in r_names] + [(A, "a4096"), (A, "a4097"), (A, "a1"), (A, "atail"), (A, "filler"), (B, "last"), (B, "uneven")]:
        add("docset(%s.%s)" % (COLUMN_NAMES[col], x), ds(col, x))
        add("NOT docset(%s.%s)" % (COLUMN_NAMES[col], x), ds(col, x, True))
        add("b.every & docset(%s.%s)" % (COLUMN_NAMES[col], x), and_(eq(B, "every"), ds(col, x)))
    add("g.7 & NOT docset(r.full)", and_(eq(G, "7"), ds(R, "full", True)))
    # ... and as the null value vectors of two columns
    for c in (NR, NA):
        add("%s IS NULL" % COLUMN_NAMES[c], null(c))
        add("%s IS NOT NULL" % COLUMN_NAMES[c], null(c, True))
        add("%s IS NULL & b.every" % COLUMN_NAMES[c], and_(null(c), eq(B, "every")))
        add("%s IS NOT NULL & g.7" % COLUMN_NAMES[c], and_(null(c, True), eq(G, "7")))
    return out


GROUP_BY_LABELS = ("a.a513 & b.every & g.5", "r IN (arr3, bit3, run3) & b.every", "b.uneven & a.filler", "r != full & b.every", "r.mix & b.every",
                   "g IN 17 & b.every", "r.rtail & a.atail", "NOT r.full", "docset(r.mix)", "nr IS NULL & b.every")
ALL_LISTS_LABELS = ("a.a9 & b.every", "a.a1 & b.firstlast", "r.rtail & a.atail", "a.a4096 & b.every", "b.every & a.filler", "r.full & a.a511",
                    "r IN (arr3, bit3, run3) & b.every", "b.late & g.5", "r != full & g.7", "a.atail", "65 postings")


def queries(seg):
    """The corpus queries a segment can name, in a fixed order: COUNT(*) for every filter, one of the three aggregation lists by
    rotation, all three for ALL_LISTS_LABELS, and SUM(v), COUNT(*) GROUP BY g for GROUP_BY_LABELS."""
    out = []
    for i, (label, f) in enumerate(filters()):
        if not available(seg, f):
            continue
        out.append(Query(label, f, COUNT_ONLY))
        lists = AGG_LISTS if label in ALL_LISTS_LABELS else [AGG_LISTS[i % 3]]
        for aggs in lists:
            out.append(Query(label, f, aggs))
        if label in GROUP_BY_LABELS:
            out.append(Query(label, f, [(Q.SUM, V), (Q.COUNT, -1)], group_by=[G]))
    return out


SKIP_POSTINGS = ("head", "gap", "far")


def skip_queries(seg):
    """The postings that skip windows, against a posting of every window: what the eleven-window segment is for."""
    out = []
    for x in SKIP_POSTINGS:
        for label, f in (("a.%s & g.5" % x, and_(eq(A, x), eq(G, "5"))), ("a.%s" % x, eq(A, x)), ("a != %s & g.5" % x, and_(ne(A, x), eq(G, "5"))),
                         ("a.%s & a.filler" % x, and_(eq(A, x), eq(A, "filler"))), ("a IN (%s, atail) & g NOT IN 16" % x, and_(in_(A, [x, "atail"]), grange(0, 16, True)))):
            out += [Query(label, f, COUNT_ONLY), Query(label, f, SUM_V), Query(label, f, THREE_COLUMNS)]
    return out


def batch_queries(seg):
    """The index-led queries of the corpus (what index_and_batch_kernel takes): no GROUP BY, at most two aggregated columns."""
    return [q for q in queries(seg) if q.index_led and not q.group_by and q.aggs != THREE_COLUMNS]


# ================================================================================================================================
# the model
# ================================================================================================================================
def mask_words(m):
    bits = np.zeros(((m.shape[0] + 63) // 64) * 64, dtype=np.uint8)
    bits[:m.shape[0]] = m
    return np.packbits(bits, bitorder="little").view(np.uint64)


def aggregate(seg, m, aggs):
    """[(count, sum, min, max)] per aggregation over the docs of mask m (None where the function does not define the field)."""
    out = []
    cnt = int(m.sum())
    for fn, col in aggs:
        if fn == Q.COUNT:
            out.append((cnt, None, None, None))
            continue
        vals = seg.values(col)[m]
        out.append((cnt, int(vals.sum()) if fn in (Q.SUM, Q.AVG) else None,
                    (float(vals.min()) if cnt else float("inf")) if fn == Q.MIN else None,
                    (float(vals.max()) if cnt else float("-inf")) if fn == Q.MAX else None))
    return out


def model(seg, query):
    """{"mask", "count", "aggs", "groups": {g dictId: aggs}} of one query."""
    m = mask(seg, query.flt)
    out = {"mask": m, "count": int(m.sum()), "aggs": aggregate(seg, m, query.aggs) if not query.group_by else None, "groups": None}
    if query.group_by:
        assert query.group_by == [G]
        out["groups"] = {int(g): aggregate(seg, m & (seg.ids[G] == g), query.aggs) for g in np.unique(seg.ids[G][m])}
    return out


def assert_matches_model(res, want, query, where=""):
    """A Result (the engine's or the oracle's) against model()'s answer, exactly."""
    def same(values, rows):
        for v, (fn, _), (cnt, s, mn, mx) in zip(values, query.aggs, rows):
            assert v.count == cnt, "%s %s: count %d != %d" % (where, query.label, v.count, cnt)
            if s is not None:
                assert v.sum_i64 == s and v.sum == float(s), "%s %s: sum %d != %d" % (where, query.label, v.sum_i64, s)
            if mn is not None:
                assert v.min == mn, "%s %s: min %r != %r" % (where, query.label, v.min, mn)
            if mx is not None:
                assert v.max == mx, "%s %s: max %r != %r" % (where, query.label, v.max, mx)
    assert res.stats[0] == want["count"] and res.stats[3] == want["mask"].shape[0], "%s %s: stats %r, %d docs match" % (where, query.label, res.stats, want["count"])
    if query.group_by:
        assert sorted(res.groups) == sorted(want["groups"]), "%s %s: groups differ" % (where, query.label)
        for g, rows in want["groups"].items():
            same(res.groups[g], rows)
    else:
        same(res.aggregations, want["aggs"])
