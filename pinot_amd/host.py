"""Python handle over the C++ host mirror (libpinot_host.so): SQL in, results blocks out.

Plays the role of the reference's test harness `BaseQueriesTest.getOperator(sql)` / `getBrokerResponse(sql, planMaker)`
(pinot-core/src/test/java/org/apache/pinot/queries/BaseQueriesTest.java:100-105,154-156): the query is parsed, lowered
with dictionary binary searches and planned by the C++ `GpuPlanMaker`, executed through the C ABI on the device, and the
per-segment blocks are merged by the C++ combine step.
"""
import ctypes as C
import json

from . import _abi
from .segment import load_host_library


class HostError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status   # 1 bad query, 2 not offloadable (keep the CPU plan), 3 runtime


def _lib():
    lib = load_host_library()
    if getattr(lib, "_host_bound", False):
        return lib
    vp = C.c_void_p
    lib.ph_last_error.restype = C.c_char_p
    lib.ph_free.argtypes = [vp]
    lib.ph_segment_create.restype = vp
    lib.ph_segment_create.argtypes = [C.c_char_p, C.c_int32]
    lib.ph_segment_add_int_column.restype = C.c_int32
    lib.ph_segment_add_int_column.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64]
    lib.ph_segment_add_numeric_column.restype = C.c_int32
    lib.ph_segment_add_numeric_column.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64]
    lib.ph_segment_add_string_column.restype = C.c_int32
    lib.ph_segment_add_string_column.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32, vp, C.c_uint64, C.c_char_p, vp, C.c_uint64]
    lib.ph_segment_set_null_vector.restype = C.c_int32
    lib.ph_segment_set_null_vector.argtypes = [vp, C.c_char_p, vp, C.c_uint64]
    lib.ph_segment_load.restype = C.c_int32
    lib.ph_segment_load.argtypes = [vp, C.c_int32]
    lib.ph_segment_destroy.argtypes = [vp]
    lib.ph_plan_maker_init.restype = C.c_int32
    lib.ph_plan_maker_init.argtypes = [C.c_int32, C.c_int32]
    lib.ph_segment_load_directory.restype = vp
    lib.ph_segment_load_directory.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]
    lib.ph_segment_describe.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.ph_plan_maker_placement.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int32)]
    for name in ("ph_parse_sql", "ph_lower_predicate", "ph_execute_sql", "ph_segment_describe", "ph_plan_maker_placement"):
        getattr(lib, name).restype = vp
    lib.ph_parse_sql.argtypes = [C.c_char_p, C.POINTER(C.c_int32)]
    lib.ph_lower_predicate.argtypes = [C.c_char_p, vp, C.c_int32, C.POINTER(C.c_int32)]
    lib.ph_execute_sql.argtypes = [C.POINTER(vp), C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]
    lib._host_bound = True
    return lib


def _take_json(lib, ptr, status):
    if status.value != 0 or not ptr:
        raise HostError(status.value, (lib.ph_last_error() or b"").decode("utf-8", "replace"))
    try:
        return json.loads(C.string_at(ptr).decode("utf-8"))
    finally:
        lib.ph_free(ptr)


def parse_sql(sql):
    lib = _lib()
    st = C.c_int32()
    return _take_json(lib, lib.ph_parse_sql(sql.encode(), C.byref(st)), st)


def lower_predicate(predicate_sql, dictionary_bytes, cardinality):
    lib = _lib()
    st = C.c_int32()
    return _take_json(lib, lib.ph_lower_predicate(predicate_sql.encode(), dictionary_bytes.ctypes.data, cardinality, C.byref(st)), st)


def placement(devices_text, segment_bytes):
    """GpuPlanMaker's gpu.devices parsing + least-loaded placement (no device touched): {"devices": [...], "placement": [...]}.
    A negative entry -(device << 48 | bytes) gives bytes back (placement -1)."""
    lib = _lib()
    st = C.c_int32()
    arr = (C.c_int64 * max(len(segment_bytes), 1))(*segment_bytes)
    return _take_json(lib, lib.ph_plan_maker_placement(devices_text.encode(), arr, len(segment_bytes), C.byref(st)), st)


def init_plan_maker(device=0, time_kernels=True):
    lib = _lib()
    st = lib.ph_plan_maker_init(device, int(time_kernels))
    if st != 0:
        raise HostError(st, (lib.ph_last_error() or b"").decode())


def _attach_null_vectors(lib, handle, columns):
    for c in columns:
        if getattr(c, "null_vector", None) is not None:
            st = lib.ph_segment_set_null_vector(handle, c.name.encode(), c.null_vector.ctypes.data, c.null_vector.nbytes)
            if st != 0:
                raise HostError(st, lib.ph_last_error().decode())


class HostSegment:
    """ImmutableSegment of the C++ host mirror built from a `SegmentData` (buffers stay owned by the SegmentData)."""

    def __init__(self, segment_data, string_dicts=None, device=0, load=True):
        """load=False: the host-side segment only (data sources, dictionaries, sorted / inverted index metadata), nothing on a device --
        enough for parse / plan inspection (`explain_filter`)."""
        lib = _lib()
        self.lib = lib
        self.data = segment_data
        self.handle = C.c_void_p(lib.ph_segment_create(segment_data.name.encode(), segment_data.num_docs))
        string_dicts = string_dicts or {}
        for c in segment_data.columns:
            inv_ptr = c.inverted.ctypes.data if c.inverted is not None else None
            inv_size = c.inverted.nbytes if c.inverted is not None else 0
            if c.name in string_dicts:
                values = b"".join(s.encode("utf-8") + b"\0" for s in string_dicts[c.name])
                st = lib.ph_segment_add_string_column(self.handle, c.name.encode(), c.bits, c.cardinality, c.fwd.ctypes.data, c.fwd.nbytes,
                                                      values, inv_ptr, inv_size)
            else:
                has_dict = c.encoding == _abi.PG_FWD_FIXED_BIT_DICT
                st = lib.ph_segment_add_numeric_column(self.handle, c.name.encode(), c.stored_type, int(has_dict), c.bits, c.cardinality,
                                                       c.fwd.ctypes.data, c.fwd.nbytes, c.dictionary.ctypes.data if has_dict else None,
                                                       c.dictionary.nbytes if has_dict else 0, inv_ptr, inv_size)
            if st != 0:
                raise HostError(st, (lib.ph_last_error() or b"").decode())
        _attach_null_vectors(lib, self.handle, segment_data.columns)
        if load:
            st = lib.ph_segment_load(self.handle, device)
            if st != 0:
                raise HostError(st, (lib.ph_last_error() or b"").decode())

    def set_queryable_doc_ids(self, doc_ids):
        """The segment's queryable (valid) docIds, as an upsert / dedup table's metadata manager publishes them (ascending docIds, or a bool
        mask); None clears them.  Every query over the segment then runs behind AND(filter, BITMAP(queryableDocIds))."""
        import numpy as np
        self.lib.ph_segment_set_queryable_doc_ids.restype = C.c_int32
        self.lib.ph_segment_set_queryable_doc_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        if doc_ids is None:
            st = self.lib.ph_segment_set_queryable_doc_ids(self.handle, None, 0)
        else:
            from .segment import roaring_serialize
            doc_ids = np.asarray(doc_ids)
            ids = np.flatnonzero(doc_ids) if doc_ids.dtype == bool else doc_ids
            data = roaring_serialize(ids.astype(np.int32), self.data.num_docs)
            st = self.lib.ph_segment_set_queryable_doc_ids(self.handle, data.ctypes.data_as(C.c_void_p), int(data.nbytes))
        if st != 0:
            raise HostError(st, (self.lib.ph_last_error() or b"").decode())

    def destroy(self):
        if self.handle:
            self.lib.ph_segment_destroy(self.handle)
            self.handle = None


class DirectorySegment:
    """A v1 / v3 Pinot segment directory opened by the native loader (ImmutableSegmentLoader.load) and made HBM resident."""

    def __init__(self, index_dir, device=0):
        lib = _lib()
        self.lib = lib
        st = C.c_int32()
        self.handle = C.c_void_p(lib.ph_segment_load_directory(str(index_dir).encode(), device, C.byref(st)))
        if st.value != 0 or not self.handle:
            self.handle = None
            raise HostError(st.value, (lib.ph_last_error() or b"").decode("utf-8", "replace"))

    def describe(self):
        st = C.c_int32()
        return _take_json(self.lib, self.lib.ph_segment_describe(self.handle, C.byref(st)), st)

    def destroy(self):
        if self.handle:
            self.lib.ph_segment_destroy(self.handle)
            self.handle = None


def explain_filter(segment, sql):
    """The physical filter operator tree (FilterPlanNode + FilterOperatorUtils) of `sql`'s WHERE clause over `segment`, as text."""
    lib = _lib()
    lib.ph_explain_filter.restype = C.c_void_p
    lib.ph_explain_filter.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int32)]
    st = C.c_int32()
    ptr = lib.ph_explain_filter(segment.handle, sql.encode(), C.byref(st))
    if st.value != 0 or not ptr:
        raise HostError(st.value, (lib.ph_last_error() or b"").decode("utf-8", "replace"))
    try:
        return C.string_at(ptr).decode("utf-8")
    finally:
        lib.ph_free(ptr)


def raw_set_table_probe(key_bytes, members, probes):
    """Builds the LDS membership table of a PG_PRED_RAW_SET leaf from `members` (distinct bit patterns, uint64) and looks `probes` up the
    way the kernels do.  Returns (bucket count, bool array of hits); bucket count 0: no table could be built."""
    import numpy as np
    lib = _lib()
    members = np.ascontiguousarray(members, dtype=np.uint64)
    probes = np.ascontiguousarray(probes, dtype=np.uint64)
    hits = np.zeros(len(probes), dtype=np.uint8)
    lib.ph_raw_set_table_probe.restype = C.c_int32
    lib.ph_raw_set_table_probe.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    buckets = lib.ph_raw_set_table_probe(int(key_bytes), members.ctypes.data, len(members), probes.ctypes.data, len(probes), hits.ctypes.data)
    return int(buckets), hits.astype(bool)


def execute_sql(segments, sql, max_execution_threads=0):
    """Returns {"segments": [per-segment block...], "combined": block}."""
    lib = _lib()
    arr = (C.c_void_p * len(segments))(*[s.handle for s in segments])
    st = C.c_int32()
    return _take_json(lib, lib.ph_execute_sql(arr, len(segments), sql.encode(), max_execution_threads, C.byref(st)), st)


KEY_INT, KEY_LONG, KEY_FLOAT, KEY_DOUBLE, KEY_STRING = range(5)      # DataType ordinals of the key arrays (host/c_api.cpp)


def group_by_combine(sql, blocks, key_types):
    """GroupByCombineOperator + GroupByDataTableReducer over group-by blocks built on the host (no device): the IndexedTable / TableResizer
    mirror of pinot_amd/csrc/host/indexed_table.cpp.  `blocks`: one list of rows per segment, a row = (key values, cells) with one cell
    (count, sum, min, max, is_null) per aggregation of `sql`, None as a key value = NULL; the cell of a DISTINCTCOUNT function carries a sixth
    element, the segment's value set as an iterable of ints.  Returns {"combined", "reduced", "table"}."""
    lib = _lib()
    P = C.POINTER
    lib.ph_group_by_combine_sets.restype = C.c_void_p
    lib.ph_group_by_combine_sets.argtypes = [C.c_char_p, C.c_int32, P(C.c_int64), P(C.c_int32), P(C.c_int64), P(C.c_double), P(C.c_char_p), P(C.c_uint8), P(C.c_int64),
                                             P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_uint8), P(C.c_int64), P(C.c_int64), P(C.c_int32)]
    rows = [r for b in blocks for r in b]
    nk = len(key_types)
    nf = len(rows[0][1]) if rows else 1
    nr = len(rows)
    br = (C.c_int64 * max(len(blocks), 1))(*[len(b) for b in blocks])
    kt = (C.c_int32 * max(nk, 1))(*key_types)
    kl, kd, ks, kn = (C.c_int64 * max(nr * nk, 1))(), (C.c_double * max(nr * nk, 1))(), (C.c_char_p * max(nr * nk, 1))(), (C.c_uint8 * max(nr * nk, 1))()
    counts, sums = (C.c_int64 * max(nr * nf, 1))(), (C.c_double * max(nr * nf, 1))()
    mins, maxs, nulls = (C.c_double * max(nr * nf, 1))(), (C.c_double * max(nr * nf, 1))(), (C.c_uint8 * max(nr * nf, 1))()
    set_offsets, set_values = [], []
    for r, (key_values, cells) in enumerate(rows):
        for k, v in enumerate(key_values):
            at = r * nk + k
            if v is None:
                kn[at] = 1
                ks[at] = b""
            elif key_types[k] in (KEY_INT, KEY_LONG):
                kl[at] = int(v)
            elif key_types[k] == KEY_STRING:
                ks[at] = str(v).encode()
            else:
                kd[at] = float(v)
        for f, cell in enumerate(cells):
            c, s, mn, mx, is_null = cell[:5]
            at = r * nf + f
            counts[at], sums[at], mins[at], maxs[at], nulls[at] = int(c), float(s), float(mn), float(mx), int(bool(is_null))
            set_offsets.append(len(set_values))
            set_values.extend(int(v) for v in (cell[5] if len(cell) > 5 else ()))
    set_offsets.append(len(set_values))
    so, sv = (C.c_int64 * len(set_offsets))(*set_offsets), (C.c_int64 * max(len(set_values), 1))(*set_values)
    st = C.c_int32()
    return _take_json(lib, lib.ph_group_by_combine_sets(sql.encode(), len(blocks), br, kt, kl, kd, ks, kn, counts, sums, mins, maxs, nulls, so, sv, C.byref(st)), st)


def combine_counts(sql, blocks, key_types=()):
    """The combine of PERCENTILE value lists built on the host (no device): ph_combine_counts.  `blocks`: one list of rows per segment, a row =
    (key values, cells) as for group_by_combine; the cell of a PERCENTILE function carries a sixth element, the segment's list as a pair
    (values, counts) of equal-length sequences (runs in any order).  An aggregation-only `sql` takes one row with an empty key per block and
    returns {"combined"}; a GROUP BY one returns {"combined", "reduced", "resultTable"}."""
    import numpy as np
    lib = _lib()
    P = C.POINTER
    lib.ph_combine_counts.restype = C.c_void_p
    lib.ph_combine_counts.argtypes = [C.c_char_p, C.c_int32, P(C.c_int64), P(C.c_int32), P(C.c_int64), P(C.c_double), P(C.c_char_p), P(C.c_uint8), P(C.c_int64),
                                      P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_uint8), C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_int32)]
    rows = [r for b in blocks for r in b]
    nk = len(key_types)
    nf = len(rows[0][1]) if rows else 1
    nr = len(rows)
    br = (C.c_int64 * max(len(blocks), 1))(*[len(b) for b in blocks])
    kt = (C.c_int32 * max(nk, 1))(*key_types)
    kl, kd, ks, kn = (C.c_int64 * max(nr * nk, 1))(), (C.c_double * max(nr * nk, 1))(), (C.c_char_p * max(nr * nk, 1))(), (C.c_uint8 * max(nr * nk, 1))()
    counts, sums = (C.c_int64 * max(nr * nf, 1))(), (C.c_double * max(nr * nf, 1))()
    mins, maxs, nulls = (C.c_double * max(nr * nf, 1))(), (C.c_double * max(nr * nf, 1))(), (C.c_uint8 * max(nr * nf, 1))()
    offsets, values, run_counts = [0], [], []
    for r, (key_values, cells) in enumerate(rows):
        for k, v in enumerate(key_values):
            at = r * nk + k
            if v is None:
                kn[at] = 1
                ks[at] = b""
            elif key_types[k] in (KEY_INT, KEY_LONG):
                kl[at] = int(v)
            elif key_types[k] == KEY_STRING:
                ks[at] = str(v).encode()
            else:
                kd[at] = float(v)
        for f, cell in enumerate(cells):
            c, s, mn, mx, is_null = cell[:5]
            at = r * nf + f
            counts[at], sums[at], mins[at], maxs[at], nulls[at] = int(c), float(s), float(mn), float(mx), int(bool(is_null))
            if len(cell) > 5:
                values.append(np.asarray(cell[5][0], dtype=np.float64))
                run_counts.append(np.asarray(cell[5][1], dtype=np.int64))
                assert values[-1].shape == run_counts[-1].shape
            offsets.append(offsets[-1] + (len(cell[5][0]) if len(cell) > 5 else 0))
    ro = np.asarray(offsets, dtype=np.int64)
    rv = np.ascontiguousarray(np.concatenate(values) if values else np.zeros(1), dtype=np.float64)
    rc = np.ascontiguousarray(np.concatenate(run_counts) if run_counts else np.zeros(1), dtype=np.int64)
    st = C.c_int32()
    return _take_json(lib, lib.ph_combine_counts(sql.encode(), len(blocks), br, kt, kl, kd, ks, kn, counts, sums, mins, maxs, nulls, ro.ctypes.data, rv.ctypes.data,
                                                 rc.ctypes.data, C.byref(st)), st)


def combine_hll(sql, blocks, key_types=()):
    """The combine of DISTINCTCOUNTHLL sketches built on the host (no device): ph_combine_hll.  `blocks` as for combine_counts; the cell of a
    DISTINCTCOUNTHLL function carries a sixth element, the segment's registers (2^log2m uint8 ranks; an empty sequence: an empty sketch)."""
    import numpy as np
    lib = _lib()
    P = C.POINTER
    lib.ph_combine_hll.restype = C.c_void_p
    lib.ph_combine_hll.argtypes = [C.c_char_p, C.c_int32, P(C.c_int64), P(C.c_int32), P(C.c_int64), P(C.c_double), P(C.c_char_p), P(C.c_uint8), P(C.c_int64),
                                   P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_uint8), C.c_void_p, C.c_void_p, P(C.c_int32)]
    rows = [r for b in blocks for r in b]
    nk = len(key_types)
    nf = len(rows[0][1]) if rows else 1
    nr = len(rows)
    br = (C.c_int64 * max(len(blocks), 1))(*[len(b) for b in blocks])
    kt = (C.c_int32 * max(nk, 1))(*key_types)
    kl, kd, ks, kn = (C.c_int64 * max(nr * nk, 1))(), (C.c_double * max(nr * nk, 1))(), (C.c_char_p * max(nr * nk, 1))(), (C.c_uint8 * max(nr * nk, 1))()
    counts, sums = (C.c_int64 * max(nr * nf, 1))(), (C.c_double * max(nr * nf, 1))()
    mins, maxs, nulls = (C.c_double * max(nr * nf, 1))(), (C.c_double * max(nr * nf, 1))(), (C.c_uint8 * max(nr * nf, 1))()
    offsets, registers = [0], []
    for r, (key_values, cells) in enumerate(rows):
        for k, v in enumerate(key_values):
            at = r * nk + k
            if v is None:
                kn[at] = 1
                ks[at] = b""
            elif key_types[k] in (KEY_INT, KEY_LONG):
                kl[at] = int(v)
            elif key_types[k] == KEY_STRING:
                ks[at] = str(v).encode()
            else:
                kd[at] = float(v)
        for f, cell in enumerate(cells):
            c, s, mn, mx, is_null = cell[:5]
            at = r * nf + f
            counts[at], sums[at], mins[at], maxs[at], nulls[at] = int(c), float(s), float(mn), float(mx), int(bool(is_null))
            regs = np.asarray(cell[5], dtype=np.uint8) if len(cell) > 5 else np.zeros(0, np.uint8)
            registers.append(regs)
            offsets.append(offsets[-1] + int(regs.shape[0]))
    ro = np.asarray(offsets, dtype=np.int64)
    rb = np.ascontiguousarray(np.concatenate(registers + [np.zeros(1, np.uint8)]), dtype=np.uint8)
    st = C.c_int32()
    return _take_json(lib, lib.ph_combine_hll(sql.encode(), len(blocks), br, kt, kl, kd, ks, kn, counts, sums, mins, maxs, nulls, ro.ctypes.data, rb.ctypes.data, C.byref(st)), st)


def combine_moments(sql, blocks, key_types=()):
    """The combine of VarianceTuples built on the host (no device): ph_combine_moments.  `blocks` as for combine_counts; the cell of a VAR_POP /
    VAR_SAMP / STDDEV_POP / STDDEV_SAMP function is (count, sum, min, max, is_null, m2): its tuple is (count, sum, m2)."""
    lib = _lib()
    P = C.POINTER
    lib.ph_combine_moments.restype = C.c_void_p
    lib.ph_combine_moments.argtypes = [C.c_char_p, C.c_int32, P(C.c_int64), P(C.c_int32), P(C.c_int64), P(C.c_double), P(C.c_char_p), P(C.c_uint8), P(C.c_int64),
                                       P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_uint8), P(C.c_double), P(C.c_int32)]
    rows = [r for b in blocks for r in b]
    nk = len(key_types)
    nf = len(rows[0][1]) if rows else 1
    nr = len(rows)
    br = (C.c_int64 * max(len(blocks), 1))(*[len(b) for b in blocks])
    kt = (C.c_int32 * max(nk, 1))(*key_types)
    kl, kd, ks, kn = (C.c_int64 * max(nr * nk, 1))(), (C.c_double * max(nr * nk, 1))(), (C.c_char_p * max(nr * nk, 1))(), (C.c_uint8 * max(nr * nk, 1))()
    counts, sums, m2s = (C.c_int64 * max(nr * nf, 1))(), (C.c_double * max(nr * nf, 1))(), (C.c_double * max(nr * nf, 1))()
    mins, maxs, nulls = (C.c_double * max(nr * nf, 1))(), (C.c_double * max(nr * nf, 1))(), (C.c_uint8 * max(nr * nf, 1))()
    for r, (key_values, cells) in enumerate(rows):
        for k, v in enumerate(key_values):
            at = r * nk + k
            if v is None:
                kn[at] = 1
                ks[at] = b""
            elif key_types[k] in (KEY_INT, KEY_LONG):
                kl[at] = int(v)
            elif key_types[k] == KEY_STRING:
                ks[at] = str(v).encode()
            else:
                kd[at] = float(v)
        for f, cell in enumerate(cells):
            c, s, mn, mx, is_null = cell[:5]
            at = r * nf + f
            counts[at], sums[at], mins[at], maxs[at], nulls[at] = int(c), float(s), float(mn), float(mx), int(bool(is_null))
            m2s[at] = float(cell[5]) if len(cell) > 5 else 0.0
    st = C.c_int32()
    return _take_json(lib, lib.ph_combine_moments(sql.encode(), len(blocks), br, kt, kl, kd, ks, kn, counts, sums, mins, maxs, nulls, m2s, C.byref(st)), st)


def hll_cardinality(registers):
    """HyperLogLog.cardinality() of 2^log2m registers, computed by the host mirror (pinot_amd/csrc/pg_hll.h)."""
    import numpy as np
    lib = _lib()
    lib.ph_hll_cardinality.restype = C.c_int64
    lib.ph_hll_cardinality.argtypes = [C.c_void_p, C.c_int32]
    regs = np.ascontiguousarray(registers, dtype=np.uint8)
    out = int(lib.ph_hll_cardinality(regs.ctypes.data, int(regs.shape[0])))
    if out < 0:
        raise ValueError("%d registers are not a HyperLogLog" % regs.shape[0])
    return out


def hll_offer_longs(longs, log2m=8):
    """The registers (uint8, 2^log2m) after offering the int64 `longs` to an empty sketch, computed with pinot_amd/csrc/pg_hll.h -- the header the
    kernels include (ph_hll_offer_longs)."""
    import numpy as np
    lib = _lib()
    lib.ph_hll_offer_longs.restype = C.c_int32
    lib.ph_hll_offer_longs.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    longs = np.ascontiguousarray(longs, dtype=np.int64)
    out = np.zeros(1 << max(int(log2m), 0) if 0 <= int(log2m) <= 20 else 1, dtype=np.uint8)
    if lib.ph_hll_offer_longs(longs.ctypes.data, int(longs.shape[0]), int(log2m), out.ctypes.data) != 0:
        raise ValueError("log2m %d is not offloaded" % log2m)
    return out


def hll_float_bits_of_widened(double_bits):
    """pg_hll.h's hll_float_bits_of_widened: the 32 stored bits of a FLOAT dictionary entry from the bits of the double it was widened to."""
    lib = _lib()
    lib.ph_hll_float_bits_of_widened.restype = C.c_uint32
    lib.ph_hll_float_bits_of_widened.argtypes = [C.c_uint64]
    return int(lib.ph_hll_float_bits_of_widened(int(double_bits) & (2 ** 64 - 1)))


def value_counts_from_device(stored_type, value_bits, counts):
    """ValueCounts::fromDeviceValues: the runs of a raw column (pg_result_value_counts) -> PERCENTILE's list as (values float64, counts int64);
    stored_type: _abi.PG_TYPE_*.  Two LONGs that land on one double are one run."""
    import numpy as np
    lib = _lib()
    bits = np.ascontiguousarray(value_bits, dtype=np.int64)
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    assert bits.shape == cnt.shape
    out_v, out_c = np.zeros(max(len(bits), 1), dtype=np.float64), np.zeros(max(len(bits), 1), dtype=np.int64)
    lib.ph_value_counts_from_device.restype = C.c_int32
    lib.ph_value_counts_from_device.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    n = lib.ph_value_counts_from_device(int(stored_type), bits.ctypes.data, cnt.ctypes.data, len(bits), out_v.ctypes.data, out_c.ctypes.data)
    return out_v[:n], out_c[:n]


def value_set_from_device(stored_type, value_bits):
    """ValueSet::fromDeviceValues: the run values of a raw column -> DISTINCTCOUNT's set as ascending int64 images of the stored type."""
    import numpy as np
    lib = _lib()
    bits = np.ascontiguousarray(value_bits, dtype=np.int64)
    out = np.zeros(max(len(bits), 1), dtype=np.int64)
    lib.ph_value_set_from_device.restype = C.c_int32
    lib.ph_value_set_from_device.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    n = lib.ph_value_set_from_device(int(stored_type), bits.ctypes.data, len(bits), out.ctypes.data)
    return out[:n]


def execute_sql_datatable(segments, sql, max_execution_threads=0):
    """The DataTable V4 bytes a server would send the broker for `sql` over these segments (combine, then
    InstanceResponseBlock.toDataTable().toBytes(); pinot_amd/csrc/host/datatable_v4.cpp)."""
    lib = _lib()
    lib.ph_execute_sql_datatable.restype = C.POINTER(C.c_uint8)
    lib.ph_execute_sql_datatable.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    handles = (C.c_void_p * len(segments))(*[s.handle for s in segments])
    size, status = C.c_int64(), C.c_int32()
    ptr = lib.ph_execute_sql_datatable(handles, len(segments), sql.encode(), max_execution_threads, C.byref(size), C.byref(status))
    if status.value != 0 or not ptr:
        raise HostError(status.value, (lib.ph_last_error() or b"").decode("utf-8", "replace"))
    data = bytes(bytearray(ptr[:size.value]))
    lib.ph_free.argtypes = [C.c_void_p]
    lib.ph_free(C.cast(ptr, C.c_void_p))
    return data
