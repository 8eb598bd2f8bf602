"""The LDS membership table of a PG_PRED_RAW_SET leaf (pinot_amd/csrc/pg_raw_set_table.h), built by the host and probed with the kernels' own
lookup: every member is found and no non-member is, for the lists a multiplicative hash could trip over."""
import numpy as np

import raw_in_cases as R
from pinot_amd import host


def test_every_member_found_and_no_stranger():
    rng = np.random.default_rng(3)
    lists = R.adversarial_key_lists()
    assert len(lists) > 100
    for key_bytes, members in lists:
        members = np.unique(np.array(members, dtype=np.uint64))
        top = 2 ** 32 if key_bytes == 4 else 2 ** 64
        strangers = rng.integers(0, top, 100_000, dtype=np.uint64)
        near = np.concatenate([members + np.uint64(1), members - np.uint64(1), members ^ np.uint64(1 << (8 * key_bytes - 1))]) % np.uint64(top) if key_bytes == 4 else \
            np.concatenate([members + np.uint64(1), members - np.uint64(1), members ^ np.uint64(1 << 63), members ^ np.uint64(1 << 32)])
        probes = np.concatenate([members, strangers, near])
        buckets, hits = host.raw_set_table_probe(key_bytes, members, probes)
        assert buckets >= 16 and buckets & (buckets - 1) == 0 and buckets * 4 * key_bytes <= 64 * 1024, (key_bytes, len(members), buckets)
        assert np.array_equal(hits, np.isin(probes, members)), (key_bytes, len(members), members[:4])


def test_the_table_stays_small():
    """two buckets of four slots per key (at least 16): a few retries of the multiplier, not a bigger table"""
    for key_bytes in (4, 8):
        for n in (1, 2, 17, 100, 1024):
            members = np.unique(np.random.default_rng(n).integers(0, 2 ** 32 if key_bytes == 4 else 2 ** 63, n, dtype=np.uint64))
            buckets, _ = host.raw_set_table_probe(key_bytes, members, members)
            assert buckets <= max(16, 4 * len(members)), (key_bytes, n, buckets)
