"""Comparing two DEVICE results of one query with each other: a batch against the single execution (tests/test_gpu_fuzz_typed.py,
tests/test_gpu_fuzz_groups.py), one routing of a group-by against another (tests/test_gpu_fuzz_groups.py)."""
import math


def same_value(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def same_results(a, b, same_plan=True):
    """Two device Results of one query (the batch against the single execution): statistics, keys and everything exact field for field.
    (FLOAT / DOUBLE sums may be added in another order by a shared launch: both are held to the model's bound instead.)
    same_plan=False: the two ran under different routings -- numEntriesScannedInFilter is compared only where both flag it exact (an
    upper bound, as under null handling, may depend on the kernel that counted it)."""
    if same_plan:
        assert a.stats == b.stats and a.filter_entries_exact == b.filter_entries_exact
    else:
        assert (a.stats[0],) + a.stats[2:] == (b.stats[0],) + b.stats[2:], "statistics %r, %r" % (a.stats, b.stats)
        assert not (a.filter_entries_exact and b.filter_entries_exact) or a.stats[1] == b.stats[1], "numEntriesScannedInFilter %d, %d" % (a.stats[1], b.stats[1])
    assert a.group_keys == b.group_keys and a.num_groups_limit_reached == b.num_groups_limit_reached
    rows = [(a.aggregations, b.aggregations)] + [(a.groups[g], b.groups[g]) for g in a.groups]
    for va, vb in rows:
        assert len(va) == len(vb)
        for x, y in zip(va, vb):
            assert x.count == y.count and x.sum_i64 == y.sum_i64 and x.sum_exact == y.sum_exact
            assert same_value(x.min, y.min) and same_value(x.max, y.max)
            assert not x.sum_exact or x.sum == y.sum
