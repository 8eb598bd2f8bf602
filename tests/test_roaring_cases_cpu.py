"""The constructed Roaring corpus (tests/roaring_cases.py) without a GPU: the census names every container shape the device tests rely on,
the oracle -- which reads the same serialized bytes with its own reader -- equals the numpy model on every corpus query, and
S.roaring_serialize round-trips the docs of every posting (the doc-set and null-vector input)."""
import numpy as np
import pytest

from oracle import oracle
from pinot_amd import segment as S
import roaring_cases as RC

BUILDS = (True, False)


@pytest.fixture(scope="module")
def rows():
    """(segment key, run_optimize, column, dictId, key, kind, cardinality, runs, lead) of every container of the single-query segments."""
    out = []
    for key in RC.SINGLE:
        for opt in BUILDS:
            seg = RC.segment(key, opt)
            for col in (RC.A, RC.B, RC.R, RC.G):
                out += [(key, opt, col) + r for r in RC.census(seg.data.columns[col])]
    return out


def having(rows, **want):
    names = ("segment", "opt", "col", "d", "key", "kind", "card", "runs", "lead")
    return [r for r in rows if all(r[names.index(k)] == v for k, v in want.items())]


@pytest.mark.parametrize("kind", [RC.ARRAY, RC.BITSET, RC.RUN])
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_every_container_kind_at_every_byte_lead(rows, kind, lead):
    assert having(rows, kind=kind, lead=lead), "no %s container at lead %d" % (kind, lead)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_the_bitset_met_by_a_multi_posting_child_at_every_lead(rows, lead):
    """and_or_bitset: r.bit3 (window 3, beside r.arr3 and r.run3), r's filler, a.a4097 and b.every / b.low are members of IN children."""
    def member(r):
        names = RC.segment(r[0], r[1]).names
        return (r[2], r[3]) in {(RC.R, names[RC.R].get("bit3")), (RC.R, 0), (RC.A, names[RC.A].get("a4097")), (RC.B, names[RC.B].get("every")),
                                (RC.B, names[RC.B].get("low"))}
    assert [r for r in having(rows, kind=RC.BITSET, lead=lead) if member(r)], "no IN-member bitset at lead %d" % lead


@pytest.mark.parametrize("card", [1, 7, 8, 9, 511, 512, 513, 4095, 4096])
@pytest.mark.parametrize("opt", BUILDS)
def test_array_cardinalities(rows, card, opt):
    assert having(rows, segment="main", opt=opt, col=RC.A, kind=RC.ARRAY, card=card)


@pytest.mark.parametrize("left", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("opt", BUILDS)
def test_every_length_of_an_arrays_last_piece(rows, left, opt):
    """and_scatter8_some: the lane that holds an array's end scatters 1 .. 8 docs; the posting is named, so it is queried on its own."""
    seg = RC.segment("main", opt)
    named = {seg.dict_id(RC.A, x) for x, _ in RC.RECIPE_A if seg.has(RC.A, x)}
    assert [r for r in having(rows, segment="main", opt=opt, col=RC.A, kind=RC.ARRAY) if r[3] in named and (r[6] - 1) % 8 + 1 == left]


def test_bitset_cardinalities(rows):
    for opt in BUILDS:
        assert having(rows, segment="main", opt=opt, col=RC.A, kind=RC.BITSET, card=4097)
    assert having(rows, segment="main", opt=False, col=RC.R, kind=RC.BITSET, card=65536)


def run_pairs(seg, name):
    """[(window, [(start, last)])] of the run containers of posting r.<name>, from the index bytes."""
    col = seg.data.columns[RC.R]
    start, length = RC.posting_slices(col)[seg.dict_id(RC.R, name)]
    out = []
    for key, kind, card, nr, off, docs in RC.parse_bitmap(col.inverted, start, length):
        if kind == RC.RUN:
            cuts = np.flatnonzero(np.diff(docs) != 1)
            firsts, lasts = np.concatenate([[0], cuts + 1]), np.concatenate([cuts, [len(docs) - 1]])
            assert len(firsts) == nr
            out.append((key, [(int(docs[a]), int(docs[b])) for a, b in zip(firsts, lasts)]))
    return out


def test_run_shapes():
    seg = RC.segment("main", True)
    assert run_pairs(seg, "full") == [(4, [(0, 65535)])]                                   # one run of the whole window
    (w, edges), = run_pairs(seg, "edges")
    assert w == 0 and edges == [(0, 3000), (5000, 5000), (60000, 65535)]                   # from doc 0; of length 1; to doc 65535
    by_window = dict(run_pairs(seg, "r65"))
    assert len(by_window[1]) == 65 and len(by_window[3]) == 130                            # a second and a third trip of the 64-lane loop
    (w, r2047), = run_pairs(seg, "r2047")
    assert len(r2047) == 2047 and all(b - a == 2 for a, b in r2047)
    (w, rtail), = run_pairs(seg, "rtail")
    assert w == 5 and rtail[-1][1] == seg.n - 5 * RC.W - 1                                 # ends on the segment's last doc
    assert len(dict(run_pairs(seg, "mix"))[2]) == 70


def windows_of(rows, seg, col, name, opt=True):
    return sorted(r[4] for r in having(rows, segment="main", opt=opt, col=col, d=seg.dict_id(col, name)))


@pytest.mark.parametrize("name,windows", [("first", [0]), ("last", [5]), ("firstlast", [0, 5]), ("high", [3, 4, 5]), ("low", [0, 1, 2]),
                                          ("evens", [0, 2, 4]), ("odds", [1, 3, 5]), ("every", [0, 1, 2, 3, 4, 5]), ("uneven", [0, 1, 5]),
                                          ("late", [0, 3, 4, 5])])
def test_window_presence_patterns(rows, name, windows):
    assert windows_of(rows, RC.segment("main", True), RC.B, name) == windows


def test_one_posting_with_another_kind_or_nothing_in_every_window(rows):
    seg = RC.segment("main", True)
    got = {r[4]: r[5] for r in having(rows, segment="main", opt=True, col=RC.R, d=seg.dict_id(RC.R, "mix"))}
    assert got == {0: RC.ARRAY, 1: RC.BITSET, 2: RC.RUN, 3: RC.ARRAY, 5: RC.RUN}


def test_one_window_with_an_array_a_bitset_and_a_run_container_of_one_column(rows):
    seg = RC.segment("main", True)
    kinds = {name: having(rows, segment="main", opt=True, col=RC.R, key=3, d=seg.dict_id(RC.R, name))[0][5] for name in ("arr3", "bit3", "run3")}
    assert kinds == {"arr3": RC.ARRAY, "bit3": RC.BITSET, "run3": RC.RUN}


@pytest.mark.parametrize("opt", BUILDS)
@pytest.mark.parametrize("key", RC.SINGLE)
def test_the_index_buffer_ends_inside_a_lanes_load(rows, key, opt):
    """The last container of the last posting of column a is an array whose last 16-byte piece is partial."""
    seg = RC.segment(key, opt)
    last = having(rows, segment=key, opt=opt, col=RC.A)[-1]
    assert last[3] == seg.data.columns[RC.A].cardinality - 1 and last[5] == RC.ARRAY and (2 * last[6]) % 16 != 0


def searches(keys, windows):
    """{(side of the guess, directory entries searched, found)} over every window, for a posting with containers in `keys` -- the
    arithmetic of and_guess_slot / and_resolve (pg_index_and.h) restated."""
    out, count = set(), len(keys)
    for key in range(windows):
        slot = min(int(np.float32(key) * (np.float32(count) / np.float32(windows))), count - 1)
        if keys[slot] == key:
            continue
        if keys[slot] < key:
            lo, hi = slot + 1, min(count - 1, slot + key - keys[slot])
        else:
            lo, hi = max(0, slot - (keys[slot] - key)), slot - 1
        out.add(("right" if keys[slot] < key else "left", max(hi - lo + 1, 0), key in keys))
    return out


def test_the_search_behind_a_missed_guess(rows):
    """In six windows no posting can make and_resolve search more than ONE directory entry (enumerated below), which is why the corpus has
    an eleven-window segment: there a.head is found after a search over three entries, a.gap is not found after one over three, and
    a.far is found over two to the left of the guess.  The six-window patterns still reach the miss branch on both sides."""
    assert max(n for windows in range(1, 7) for present in range(1, 1 << windows)
               for _, n, _ in searches([w for w in range(windows) if (present >> w) & 1], windows)) == 1
    seg = RC.segment("skip", True)
    assert seg.windows == 11
    keys = {x: sorted(r[1] for r in RC.census(seg.data.columns[RC.A]) if r[0] == seg.dict_id(RC.A, x)) for x in RC.SKIP_POSTINGS}
    assert keys == {"head": [0, 1, 2, 3, 4], "gap": [0, 1, 2, 3, 5], "far": [1, 8, 10]}
    assert ("right", 3, True) in searches(keys["head"], 11)
    assert ("right", 3, False) in searches(keys["gap"], 11)
    assert ("left", 2, True) in searches(keys["far"], 11)
    six = set()
    for x in ("uneven", "late", "high", "low"):
        six |= searches(windows_of(rows, RC.segment("main", True), RC.B, x), 6)
    assert {("right", 1, True), ("left", 1, True), ("right", 0, False), ("left", 0, False)} <= six, six


@pytest.mark.parametrize("opt", BUILDS)
@pytest.mark.parametrize("key", list(RC.SEGMENTS))
def test_the_oracle_equals_the_model_on_every_corpus_query(key, opt):
    seg = RC.segment(key, opt)
    qs = RC.skip_queries(seg) if key == "skip" else RC.queries(seg)
    assert len(qs) > (40 if key == "skip" else 150)
    bitmaps = {}
    for q in qs:
        want = RC.model(seg, q)
        RC.assert_matches_model(oracle.execute(seg.data, q.spec(seg)), want, q, "oracle")
        if q.label not in bitmaps:
            words, card = oracle.filter_bitmap(seg.data, q.bitmap_spec(seg))
            assert card == want["count"] and np.array_equal(words, RC.mask_words(want["mask"])), q.label
            bitmaps[q.label] = True


def test_the_aggregation_lists_meet_both_sides_of_the_gather_rule():
    seg = RC.segment("main", True)
    qs = [q for q in RC.queries(seg) if q.aggs in (RC.SUM_V, RC.FIVE_V) and q.index_led and not q.group_by]
    assert any(q.certainly_gathered(seg) for q in qs)
    # expected docs of `b.every & a.filler` are far above four per window: the bitmap -> scan path
    assert any(q.label == "b.every & a.filler" and RC.model(seg, q)["count"] > 1000 * seg.windows for q in qs)


@pytest.mark.parametrize("opt", BUILDS)
def test_roaring_serialize_round_trips_every_posting(opt):
    seg = RC.segment("main", True)
    for col in (RC.A, RC.B, RC.R):
        column = seg.data.columns[col]
        for d in range(column.cardinality):
            docs = np.flatnonzero(seg.ids[col] == d)
            assert np.array_equal(RC.posting_docs(column, d), docs)                       # the index bytes hold the recipe
            assert np.array_equal(RC.bitmap_docs(S.roaring_serialize(docs.astype(np.int32), seg.n, run_optimize=opt)), docs)
    for c, m in seg.nulls.items():
        assert np.array_equal(RC.bitmap_docs(seg.data.columns[c].null_vector), np.flatnonzero(m))
