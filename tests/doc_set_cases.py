"""Case builder of the doc-set tests (PG_PRED_DOC_SET: the queryable docIds of an upsert / dedup segment as a filter leaf).

The yardstick is the unchanged oracle over a TWIN segment: a doc set V equals an inverted-index leaf `= 1` on a synthetic two-value
dictionary column (dictionary {0, 1}, dictId = 1 where the doc is in V) appended behind the segment's own columns.  The reference builds
the same operator class for both -- bitmap based, priority 100 (FilterOperatorUtils.java:222-224), no entries scanned, the same
FastFilteredCountOperator rule -- so docs, aggregates and all four statistics of a query over (segment, V) are those of the rewritten query
over the twin.  The engine's segment never gets that column.

Nothing here needs a GPU: tests/test_doc_set_cpu.py pins the twin to a numpy model, tests/test_gpu_doc_set.py holds the device to the twin."""
import numpy as np

import fuzz_cases as F
from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S

VALID_COLUMN = "$validDocIds"


def valid_column(mask, name=VALID_COLUMN):
    """The synthetic column: dictionary {0, 1} (always both entries, also when V is empty or holds every doc), inverted index."""
    return S.Column.from_dict_ids(name, np.array([0, 1], dtype=np.int32), np.asarray(mask, dtype=bool).astype(np.int32), with_inverted=True)


def twin_segment(seg, masks):
    """`seg` (S.SegmentData) with one synthetic column per doc set appended, in the order of `masks`."""
    cols = list(seg.columns) + [valid_column(m, VALID_COLUMN + (str(i) if i else "")) for i, m in enumerate(masks)]
    twin = S.SegmentData(seg.name, seg.num_docs, cols)
    if hasattr(seg, "string_dicts"):
        twin.string_dicts = seg.string_dicts
    return twin


def twin_pred(column, exclusive=False):
    """The inverted leaf `synthetic column = 1` (exclusive: `!= 1`, the flipped bitmap)."""
    return Q.Pred.dict_range(column, 1, 2, exclusive=exclusive, inverted=True)


def to_twin(spec, column_of_id):
    """`spec` with every Pred.doc_set(id) rewritten into the inverted leaf on twin column column_of_id[id].  One Pred object behind several
    leaves stays one Pred object."""
    rewritten = {}

    def pred(p):
        if id(p) not in rewritten:
            rewritten[id(p)] = twin_pred(column_of_id[p.lo], p.exclusive) if p.kind == _abi.PG_PRED_DOC_SET else p
        return rewritten[id(p)]

    def walk(n):
        if n.op == _abi.PG_FILTER_LEAF:
            return Q.leaf(pred(n.pred))
        return Q.Node(n.op, [walk(ch) for ch in n.children])

    return Q.QuerySpec(spec.aggregations, filter=walk(spec.filter) if spec.filter is not None else None, group_by=spec.group_by,
                       null_handling=spec.null_handling, num_groups_limit=spec.num_groups_limit, stats_upper_bound_ok=spec.stats_upper_bound_ok)


def with_valid(flt, valid_leaf):
    """FilterPlanNode.java:92-103: AND(user filter, queryable docIds), in that child order; without a user filter the leaf alone."""
    return valid_leaf if flt is None else Q.and_(flt, valid_leaf)


def mask_words(mask):
    return F.mask_words(np.asarray(mask, dtype=bool))


def random_mask(rng, n, density):
    if density <= 0.0:
        return np.zeros(n, bool)
    if density >= 1.0:
        return np.ones(n, bool)
    return rng.random(n) < density


# ---- the typed fuzz (tests/fuzz_cases.py) behind doc sets ----
MASK_STYLES = ["half", "sparse", "dense", "run", "all", "none"]


def fuzz_masks(seg):
    """Two doc sets per fuzz segment: V (goes to the root of every tree) and W (goes to a random inner position)."""
    rng = np.random.default_rng(123_000 + F.SEED_BASE + seg.seed)
    out = []
    for _ in range(2):
        style = MASK_STYLES[int(rng.integers(0, len(MASK_STYLES)))]
        n = seg.n
        if style == "run":
            m = np.zeros(n, bool)
            m[n // 4: n // 4 + max(1, n // 2)] = True
        else:
            m = random_mask(rng, n, {"half": 0.5, "sparse": 0.01, "dense": 0.97, "all": 1.0, "none": 0.0}[style])
        out.append(m)
    return out


def twin_fuzz_segment(seg, masks):
    """F.Segment whose columns are seg's plus the synthetic ones (the model and the oracle both read it)."""
    cols = list(seg.cols)
    for i, m in enumerate(masks):
        column = valid_column(m, VALID_COLUMN + (str(i) if i else ""))
        ids = np.asarray(m, dtype=bool).astype(np.int32)
        cols.append(F.Col(column.name, F.DICT_INT, ids.copy(), column, ids=ids, dict_values=np.array([0, 1], dtype=np.int32), pool="benign"))
    twin = F.Segment(seg.seed, seg.n, cols)
    return twin


def _count_leaves(t):
    return 1 if t[0] == "leaf" else sum(_count_leaves(ch) for ch in t[1])


def _positions(t, path=()):
    out = [path]
    if t[0] != "leaf":
        for i, ch in enumerate(t[1]):
            out += _positions(ch, path + (i,))
    return out


def _replace(t, path, fn):
    if not path:
        return fn(t)
    kids = list(t[1])
    kids[path[0]] = _replace(kids[path[0]], path[1:], fn)
    return (t[0], kids)


def wrap_fuzz_query(rng, fq, leaf_v, leaf_w_of):
    """The generated query behind doc sets: AND(tree, V) at the root (V alone without a tree), and -- where the leaf table has room -- W
    and-ed or or-ed to the subtree at a random position INSIDE the user's tree.  leaf_v: the F.Leaf of V; leaf_w_of(exclusive): the one of W.
    Returns (FuzzQuery, shape) with shape "single" (V is the whole filter), "root" (V at the root only) or "inner"."""
    tree, shape = fq.tree, "single"
    if tree is not None:
        shape = "root"
        if _count_leaves(tree) + 2 <= F.MAX_LEAVES and rng.integers(0, 2):
            path = F._pick(rng, _positions(tree))
            op = "and" if rng.integers(0, 2) else "or"
            w = leaf_w_of(bool(rng.integers(0, 3) == 0))
            tree = _replace(tree, path, lambda sub: (op, [sub, ("leaf", w)]))
            shape = "inner"
        tree = ("and", [tree, ("leaf", leaf_v)])
    else:
        tree = ("leaf", leaf_v)
    return F.FuzzQuery(fq.aggs, tree, fq.group_by, fq.null_handling, fq.limit), shape


def index_only(fq):
    """Every leaf of the tree is answered by an index or is constant: no scan leaf (numEntriesScannedInFilter is 0)."""
    return all(x.kind in ("doc_set", "doc_range", "inverted_range", "inverted_set", "is_null", "match_all", "match_none") for x in fq.leaves())


def twin_fuzz_query(fq, twin_leaf_of):
    """`fq` with its doc-set leaves replaced by the twin's inverted leaves (twin_leaf_of: F.Leaf -> F.Leaf, one twin object per leaf object)."""
    made = {}

    def walk(t):
        if t[0] == "leaf":
            leaf = t[1]
            if leaf.kind != "doc_set":
                return t
            if id(leaf) not in made:
                made[id(leaf)] = twin_leaf_of(leaf)
            return ("leaf", made[id(leaf)])
        return (t[0], [walk(ch) for ch in t[1]])

    return F.FuzzQuery(fq.aggs, walk(fq.tree), fq.group_by, fq.null_handling, fq.limit)


def device_leaf(doc_set_id, which, exclusive=False):
    return F.Leaf("doc_set", Q.Pred.doc_set(doc_set_id, exclusive), column=-1, exclusive=exclusive, which=which)


def twin_leaf(twin_column, exclusive=False):
    return F.Leaf("inverted_range", twin_pred(twin_column, exclusive), column=twin_column, exclusive=exclusive, lo=1, hi=2)
