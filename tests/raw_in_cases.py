"""Shared by the CPU and GPU tests of IN / NOT IN on raw (no-dictionary) INT / LONG / FLOAT / DOUBLE columns (PG_PRED_RAW_SET: the
reference's Int / Long / Float / DoubleRawValueBasedInPredicateEvaluator, InPredicateEvaluatorFactory.java:74-107, under a
ScanBasedFilterOperator).

A scan leaf's result does not depend on how its column is encoded, so every case has a TWIN segment in which the filtered columns are
dictionary-encoded and the predicate is a scan PG_PRED_DICT_SET over the dictIds of the listed values; everything else is identical.
The device runs the raw segment with PG_PRED_RAW_SET, the oracle the twin.  (The oracle has a PG_PRED_RAW_SET leaf of its own as well --
the typed fuzz, tests/fuzz_cases.py, needs the reference side to answer every generated query -- and tests/test_oracle_raw_in.py pins
it to numpy and to this twin yardstick.)"""
import numpy as np

from pinot_amd import _abi
from pinot_amd import query as Q
from pinot_amd import segment as S

CAP = _abi.PG_RAW_SET_MAX_VALUES
DTYPES = {"ri": np.int32, "rl": np.int64, "rf": np.float32, "rd": np.float64}
FILTER_COLUMNS = ("ri", "rl", "rf", "rd")            # raw INT / LONG / FLOAT / DOUBLE, columns 0..3
# aggregated columns: 4 ai raw INT, 5 al raw LONG, 6 ad raw DOUBLE, 7 dv dictionary INT; 8 f dictionary (range leaves), 9 gk dictionary key,
# 10 rk raw INT key, 11 s sorted dictionary column, 12 iv dictionary column with an inverted index
AI, AL, AD, DV, F, GK, RK, SORTED, INV = 4, 5, 6, 7, 8, 9, 10, 11, 12


def column_values(n, seed=0, distinct=1500):
    """The four filter columns' values: `distinct` different values each, drawn from a pool that holds the type's extremes."""
    rng = np.random.default_rng(seed + 11)
    pools = {
        "ri": np.unique(np.concatenate([rng.integers(-2 ** 31, 2 ** 31, distinct, dtype=np.int64), [-1, 0, 1, -2 ** 31, 2 ** 31 - 1]])).astype(np.int32),
        "rl": np.unique(np.concatenate([rng.integers(-2 ** 63, 2 ** 63 - 1, distinct, dtype=np.int64), [-1, 0, 1, -2 ** 63, 2 ** 63 - 1, 2 ** 32, -2 ** 32]])).astype(np.int64),
        "rf": np.unique(np.concatenate([rng.normal(0, 1e3, distinct).astype(np.float32), np.float32([np.inf, -np.inf, 1e-45, -1e-45, 3.4028235e38, 0.1, 1.0])])).astype(np.float32),
        "rd": np.unique(np.concatenate([rng.normal(0, 1e6, distinct), [np.inf, -np.inf, 5e-324, -5e-324, 1.7976931348623157e308, 0.1, 1.0]])).astype(np.float64),
    }
    return {k: p[rng.integers(0, len(p), n)] if n else p[:0] for k, p in pools.items()}, pools


def segments(n, seed=0, null_mask=None, distinct=1500):
    """-> (raw SegmentData, twin SegmentData, {column name: its values}).  The twin's ri / rl / rf / rd are dictionary columns."""
    vals, _ = column_values(n, seed, distinct)
    rng = np.random.default_rng(seed + 12)
    extra = {
        "ai": rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int32),
        "al": rng.integers(-10 ** 12, 10 ** 12, n).astype(np.int64),
        "ad": rng.normal(0, 100, n).astype(np.float64),
        "dv": (rng.integers(0, 4000, n) * 7 - 9000).astype(np.int32),
        "f": rng.integers(0, 300, n).astype(np.int32),
        "gk": rng.integers(0, 23, n).astype(np.int32),
        "rk": (rng.integers(0, 41, n) - 20).astype(np.int32),
        "s": np.sort(rng.integers(0, 50, n)).astype(np.int32),
        "iv": rng.integers(0, 12, n).astype(np.int32),
    }

    def rest():
        return [S.Column.raw("ai", extra["ai"]), S.Column.raw_typed("al", extra["al"]), S.Column.raw_typed("ad", extra["ad"]),
                S.Column.dict_encoded("dv", extra["dv"]), S.Column.dict_encoded("f", extra["f"]), S.Column.dict_encoded("gk", extra["gk"]),
                S.Column.raw("rk", extra["rk"]), S.Column.dict_encoded("s", extra["s"]), S.Column.dict_encoded("iv", extra["iv"], with_inverted=True)]

    def nulls(col, name):
        return col.with_nulls(null_mask) if null_mask is not None and name == "ri" else col

    raw_cols = [nulls(S.Column.raw("ri", vals["ri"]) if k == "ri" else S.Column.raw_typed(k, vals[k]), k) for k in FILTER_COLUMNS]
    twin_cols = [nulls(S.Column.dict_encoded_typed(k, vals[k]), k) for k in FILTER_COLUMNS]
    all_vals = dict(vals)
    all_vals.update(extra)
    return S.SegmentData("rawin", n, raw_cols + rest()), S.SegmentData("rawin_twin", n, twin_cols + rest()), all_vals


def raw_pred(column, values, exclusive=False):
    """The PG_PRED_RAW_SET leaf of `values` on filter column `column` (0..3)."""
    name = FILTER_COLUMNS[column]
    if name in ("ri", "rl"):
        return Q.Pred.raw_set(column, [int(v) for v in values], exclusive=exclusive)
    return Q.Pred.raw_set_f64(column, [float(v) for v in values], exclusive=exclusive)      # (a float32 widens exactly)


def twin_pred(twin, column, values, exclusive=False):
    """The same list as a scan PG_PRED_DICT_SET on the twin's dictionary column.  (A raw evaluator is never constant: a list that names
    none or all of the column's values still scans every doc, so such lists stay set leaves here too.)"""
    col = twin.columns[column]
    listed = np.asarray(list(values), dtype=DTYPES[FILTER_COLUMNS[column]])
    ids = np.flatnonzero(np.isin(col.dict_values, listed)).tolist()
    return Q.Pred.dict_set(column, ids, col.cardinality, exclusive=exclusive)


def member_mask(vals, column, values):
    name = FILTER_COLUMNS[column]
    return np.isin(vals[name], np.asarray(list(values), dtype=DTYPES[name]))


def adversarial_key_lists():
    """(key bytes, member bit patterns) for the table builder: what a multiplicative hash could trip over."""
    out = [(4, [7]), (4, [7, 8]), (4, list(range(CAP))), (4, [0xFFFFFFFF, 0, 0x80000000, 0x7FFFFFFF]),
           (8, [0, 2 ** 64 - 1, 2 ** 63, 2 ** 63 - 1, 1, 2 ** 32, 2 ** 32 - 1]), (8, [7]), (8, list(range(CAP)))]
    for k in range(32):
        out.append((4, sorted({(i << k) & 0xFFFFFFFF for i in range(CAP)})))                  # arithmetic progressions, stride 2^k
        out.append((8, sorted({(i << k) for i in range(CAP)})))
        out.append((8, sorted({(i << (k + 32)) & (2 ** 64 - 1) for i in range(CAP)})))
    out.append((4, [(i * 4096 + 5) & 0xFFFFFFFF for i in range(CAP)]))                       # all equal modulo any table size
    out.append((8, [i * 2 ** 40 + 5 for i in range(CAP)]))
    f32 = np.array([np.inf, -np.inf, 1e-45, -1e-45, 1e-40, 3.4028235e38, 0.1], dtype=np.float32).view(np.uint32)
    f64 = np.array([np.inf, -np.inf, 5e-324, -5e-324, 1e-310, 1.7976931348623157e308, 0.1]).view(np.uint64)
    out.append((4, [int(x) for x in f32]))
    out.append((8, [int(x) for x in f64]))
    return out


def value_lists(pools, column, rng):
    """Lists for one filter column: sizes 1, 2, 17, 100, CAP; members present and absent, the column's min and max, duplicates."""
    name = FILTER_COLUMNS[column]
    pool = pools[name]
    dt = DTYPES[name]
    absent = {"ri": [123456789, -987654321], "rl": [2 ** 40 + 12345, -2 ** 50 - 1], "rf": [np.float32(12345.678), np.float32(-7.25e-20)],
              "rd": [12345.678901, -7.25e-200]}[name]
    lists = []
    for size in (1, 2, 17, 100, CAP):
        take = pool[rng.choice(len(pool), min(size, len(pool)), replace=False)].tolist()
        if size >= 17:
            take[0], take[1] = pool[0].item(), pool[-1].item()                # the column's smallest and largest value
            take[2], take[3] = absent
            take.append(take[4])                                              # a duplicate (the engine de-duplicates: still `size` distinct values)
        lists.append([dt(v).item() for v in take])
    return lists
