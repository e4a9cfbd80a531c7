"""Host-side mirror of the reference API for the Parse()/ParseND() path.

Reference interface mirrored here:
  simdjson_amd64.go:37  SupportedCPU()        -> supported()
  simdjson_amd64.go:66  Parse(b, reuse, opts) -> parse(b, reuse=None, copy_strings=True)
  simdjson_amd64.go:82  ParseND(...)          -> parse_nd(...)
  options.go:13         WithCopyStrings(bool) -> copy_strings keyword
  parsed_json.go:64     ParsedJson{Message, Tape, Strings} -> ParsedJson
Errors follow parse_json_amd64.go:81,93 and simdjson_amd64.go:43 (same messages).
"""
import ctypes as C

import numpy as np

from . import _lib

FLAG_NDJSON = 1
FLAG_COPY_STRINGS = 2
FLAG_KEY_FLAGS = 4  # the parse leaves the key flags MarshalJSON needs (include/sjhip.h)

ERR_STAGE1 = "Failed to find all structural indices for stage 1"
ERR_STAGE2 = "Bad parsing while executing stage 2"
ERR_NODEVICE = "Host CPU does not meet target specs"  # kept verbatim from the reference


class ParseError(Exception):
    def __init__(self, msg, code):
        super().__init__(msg)
        self.code = code


TYPE_NULL, TYPE_STRING, TYPE_INT, TYPE_UINT, TYPE_FLOAT, TYPE_BOOL, TYPE_OBJECT, TYPE_ARRAY = range(1, 9)  # SJHIP_TYPE_* (row_schema)


def supported() -> bool:
    return bool(_lib.lib().sjhip_supported())


def _pinned_view(ptr, count, ctype, dtype):
    """numpy array over `count` elements of library-owned host memory (read-only)"""
    if not count or not ptr:
        return np.empty(0, dtype=dtype)
    a = np.frombuffer((ctype * count).from_address(ptr), dtype=dtype)
    a.flags.writeable = False
    return a


class Context:
    """One per concurrent parse: owns a HIP stream and recycled device arenas
    (the role of `reuse *ParsedJson`, simdjson_amd64.go:46-51)."""

    def __init__(self, device: int = 0):
        L = _lib.lib()
        self._h = L.sjhip_ctx_create(device)
        if not self._h:
            raise ParseError(ERR_NODEVICE, 3)
        self.device = device

    def close(self):
        if self._h:
            _lib.lib().sjhip_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return _lib.lib().sjhip_last_error(self._h).decode()

    def device_bytes(self) -> int:
        """bytes of device memory the context's arenas hold right now (they only grow; see trim)"""
        return int(_lib.lib().sjhip_ctx_device_bytes(self._h))

    def trim(self):
        """give every arena back (after an unusually large message); the next parse allocates what it needs"""
        self._check(_lib.lib().sjhip_ctx_trim(self._h))

    def input_block(self, nbytes):
        """A pinned host block of the context as a writable uint8 array of `nbytes` bytes: read the input straight into
        it (file.readinto) and hand it to parse() -- the copy to the device then runs at the pinned rate."""
        p = _lib.lib().sjhip_input_block(self._h, nbytes)
        if not p:
            raise ParseError(f"sjhip_input_block: {self.last_error()}", -1)
        return np.frombuffer((C.c_uint8 * nbytes).from_address(p), dtype=np.uint8)

    def set_stream(self, stream_ptr):
        _lib.lib().sjhip_ctx_set_stream(self._h, C.c_void_p(stream_ptr or 0))

    def _check(self, rc):
        if rc == 0:
            return
        if rc == 1:
            raise ParseError(ERR_STAGE1, rc)
        if rc == 2:
            raise ParseError(ERR_STAGE2, rc)
        if rc == 3:
            raise ParseError(ERR_NODEVICE, rc)
        raise ParseError(f"sjhip error {rc}: {self.last_error()}", rc)

    # ---- stage 1 ---------------------------------------------------------------------------
    def stage1(self, data, ndjson=False):
        """findStructuralIndices on a host buffer -> (ok, uint32 positions)."""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        cap = a.size + 64
        pos = np.empty(cap, dtype=np.uint32)
        n = C.c_size_t(0)
        ok = C.c_int(0)
        rc = _lib.lib().sjhip_stage1(self._h, a.ctypes.data if a.size else None, a.size, int(ndjson),
                                     pos.ctypes.data, cap, C.byref(n), C.byref(ok))
        self._check(rc)
        return bool(ok.value), pos[: n.value].copy()

    def stage1_device(self, d_msg_ptr, length, d_pos_ptr, pos_cap, ndjson=False):
        n = C.c_size_t(0)
        ok = C.c_int(0)
        rc = _lib.lib().sjhip_stage1_device(self._h, C.c_void_p(d_msg_ptr), length, int(ndjson),
                                            C.c_void_p(d_pos_ptr), pos_cap, C.byref(n), C.byref(ok))
        self._check(rc)
        return bool(ok.value), n.value

    STAGE1_QUEUE_SLOTS = 64

    def stage1_queue(self, d_msg_ptr, length, d_pos_ptr, pos_cap, slot, ndjson=False):
        """sjhip_stage1_device without the synchronisation: the message goes behind what the stream holds (queued messages
        of one mode run several to a launch, started no later than stage1_wait()); its result is taken with
        stage1_result(slot, length) after stage1_wait()."""
        self._check(_lib.lib().sjhip_stage1_device_queue(self._h, C.c_void_p(d_msg_ptr), length, int(ndjson),
                                                         C.c_void_p(d_pos_ptr), pos_cap, int(slot)))

    def stage1_wait(self):
        self._check(_lib.lib().sjhip_stage1_device_wait(self._h))

    def stage1_result(self, slot, length):
        n = C.c_size_t(0)
        ok = C.c_int(0)
        self._check(_lib.lib().sjhip_stage1_device_result(self._h, int(slot), length, C.byref(n), C.byref(ok)))
        return bool(ok.value), n.value

    def stage1_time(self, d_msg_ptr, length, d_pos_ptr, pos_cap, iters, ndjson=False):
        ms = C.c_float(0)
        rc = _lib.lib().sjhip_stage1_time(self._h, C.c_void_p(d_msg_ptr), length, int(ndjson), C.c_void_p(d_pos_ptr),
                                          pos_cap, iters, C.byref(ms))
        self._check(rc)
        return ms.value

    # ---- whole parse -----------------------------------------------------------------------
    def parse(self, data, ndjson=False, copy_strings=True, reuse=None, view=False, key_flags=False):
        """Parse / ParseND.  `reuse`: a ParsedJson whose Tape / Strings capacity is recycled (the reference's
        `reuse *ParsedJson`, simdjson_amd64.go:46-51): its arrays are overwritten.
        `view=True`: Tape / Strings are read-only views of the context's pinned result block (sjhip_fetch_view) --
        no copy into Python-owned arrays; like a recycled ParsedJson they are overwritten by the next parse on this
        context.  `key_flags=True`: marshal_json() of this result is going to be called (SJHIP_FLAG_KEY_FLAGS)."""
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        tl, sl, mo, ml = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        flags = (FLAG_NDJSON if ndjson else 0) | (FLAG_COPY_STRINGS if copy_strings else 0) | (FLAG_KEY_FLAGS if key_flags else 0)
        L = _lib.lib()
        rc = L.sjhip_parse(self._h, a.ctypes.data if a.size else None, a.size, flags, C.byref(tl), C.byref(sl),
                           C.byref(mo), C.byref(ml))
        self._check(rc)
        msg = a[mo.value: mo.value + ml.value]  # (a view: no copy of the message on the parse path)
        if view:
            tp, sp = C.c_void_p(), C.c_void_p()
            self._check(L.sjhip_fetch_view(self._h, C.byref(tp), C.byref(sp)))
            tape = _pinned_view(tp.value, tl.value, C.c_uint64, np.uint64)
            strings = _pinned_view(sp.value, sl.value, C.c_uint8, np.uint8)
            pj = ParsedJson(msg, tape, strings)
            pj._owner = self  # the views live in this context's pinned memory
            return pj
        tape_buf = reuse._tape_buf if reuse is not None and reuse._tape_buf.size >= tl.value else \
            np.empty(tl.value, dtype=np.uint64)
        str_buf = reuse._str_buf if reuse is not None and reuse._str_buf.size >= sl.value else \
            np.empty(sl.value, dtype=np.uint8)
        rc = L.sjhip_fetch(self._h, tape_buf.ctypes.data, str_buf.ctypes.data)
        self._check(rc)
        return ParsedJson(msg, tape_buf[:tl.value], str_buf[:sl.value], tape_buf, str_buf)

    def parse_device(self, d_msg_ptr, length, ndjson=False, copy_strings=True, key_flags=False):
        tl, sl = C.c_size_t(0), C.c_size_t(0)
        flags = (FLAG_NDJSON if ndjson else 0) | (FLAG_COPY_STRINGS if copy_strings else 0) | (FLAG_KEY_FLAGS if key_flags else 0)
        rc = _lib.lib().sjhip_parse_device(self._h, C.c_void_p(d_msg_ptr), length, flags, C.byref(tl), C.byref(sl))
        self._check(rc)
        return tl.value, sl.value

    # ---- many documents, one launch set (include/sjhip.h: sjhip_parse_batch) -----------------------------------
    def parse_batch(self, docs, fetch=True):
        """Parses the documents of `docs` (bytes-like, host memory) as ONE packed ND message: document i is root i of
        the returned ParsedJson (Message = b"": every string is copied).  One invalid document fails the batch."""
        arrs = [np.frombuffer(d, dtype=np.uint8) if not isinstance(d, np.ndarray) else d for d in docs]
        n = len(arrs)
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])
        lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
        tl, sl = C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_parse_batch(self._h, ptrs, lens, n, FLAG_COPY_STRINGS, C.byref(tl), C.byref(sl)))
        if not fetch:
            return tl.value, sl.value
        tape, strings = self.fetch(tl.value, sl.value)
        return ParsedJson(b"", tape, strings)

    def parse_batch_device(self, d_buf_ptr, offs, lens):
        """The same with the documents resident in one device buffer (offs[i], lens[i]); the result stays on the device."""
        n = len(offs)
        o = (C.c_size_t * max(n, 1))(*[int(x) for x in offs])
        ln = (C.c_size_t * max(n, 1))(*[int(x) for x in lens])
        tl, sl = C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_parse_batch_device(self._h, C.c_void_p(d_buf_ptr), o, ln, n, FLAG_COPY_STRINGS,
                                                        C.byref(tl), C.byref(sl)))
        return tl.value, sl.value

    # ---- queries on the device-resident result (include/sjhip.h: sjhip_count_where / sjhip_filter_where) --------
    def count_where(self, key, value):
        """countWhere(key, value, pj) of the reference's tests (ndjson_test.go:421-471) on the device: records whose
        root object has `key` (first occurrence, top level) with the string value `value`."""
        k, v = bytes(key), bytes(value)
        n = C.c_uint64(0)
        self._check(_lib.lib().sjhip_count_where(self._h, k, len(k), v, len(v), C.byref(n)))
        return n.value

    def filter_where(self, key, value, fetch=True):
        """Compacts the matching records into a new (Tape, Strings.B) on the device -- what ParseND returns for the
        document made of the matching lines -- and fetches it.  -> (n_records, ParsedJson or None)"""
        k, v = bytes(key), bytes(value)
        n, tl, sl = C.c_uint64(0), C.c_size_t(0), C.c_size_t(0)
        L = _lib.lib()
        self._check(L.sjhip_filter_where(self._h, k, len(k), v, len(v), C.byref(n), C.byref(tl), C.byref(sl)))
        if not fetch:
            return n.value, None
        tape = np.empty(tl.value, dtype=np.uint64)
        strings = np.empty(sl.value, dtype=np.uint8)
        self._check(L.sjhip_fetch_filtered(self._h, tape.ctypes.data, strings.ctypes.data))
        return n.value, ParsedJson(b"", tape, strings)

    # ---- paths, typed values, key sets (include/sjhip.h: sjhip_find_path / _count_where_path / _project_keys) --------
    PATH_NOT_FOUND = 0xFFFFFFFFFFFFFFFF
    PATH_NOT_OBJECT = 0xFFFFFFFFFFFFFFFE
    OP_EXISTS, OP_EQ_STRING, OP_EQ_INT, OP_EQ_UINT, OP_EQ_FLOAT, OP_EQ_BOOL, OP_IS_NULL = range(7)
    (OP_LT_INT, OP_LE_INT, OP_GT_INT, OP_GE_INT, OP_LT_UINT, OP_LE_UINT, OP_GT_UINT, OP_GE_UINT,
     OP_LT_FLOAT, OP_LE_FLOAT, OP_GT_FLOAT, OP_GE_FLOAT, OP_PREFIX_STRING) = range(7, 20)
    WHERE_NOT = 1

    @staticmethod
    def _keys(keys):
        ks = [bytes(k) for k in keys]
        lens = (C.c_uint32 * max(len(ks), 1))(*[len(k) for k in ks])
        return b"".join(ks), lens, len(ks)

    def find_path(self, *path):
        """Iter.FindElement(path...) (parsed_json.go:833-865) on the root of every record of the last parse, on the device.
        -> uint64 array, one entry per record: the tape index of the element's value, PATH_NOT_FOUND or PATH_NOT_OBJECT"""
        blob, lens, n = self._keys(path)
        L = _lib.lib()
        cnt = C.c_size_t(0)
        probe = np.empty(1, dtype=np.uint64)
        L.sjhip_find_path(self._h, blob, lens, n, probe.ctypes.data, 0, C.byref(cnt))  # (no room: only the record count is set)
        out = np.empty(max(cnt.value, 1), dtype=np.uint64)
        self._check(L.sjhip_find_path(self._h, blob, lens, n, out.ctypes.data, out.size, C.byref(cnt)))
        return out[: cnt.value]

    def _op_value(self, op, value):
        """the value of a typed predicate as the bytes the C call takes: bytes for OP_EQ_STRING / OP_PREFIX_STRING, an int for the
        *_INT / *_UINT operators, a float for the *_FLOAT ones, a bool for OP_EQ_BOOL, nothing for the others"""
        import struct
        if op in (self.OP_EQ_STRING, self.OP_PREFIX_STRING):
            return bytes(value)
        if op == self.OP_EQ_INT or self.OP_LT_INT <= op <= self.OP_GE_INT:
            return struct.pack("<q", int(value))
        if op == self.OP_EQ_UINT or self.OP_LT_UINT <= op <= self.OP_GE_UINT:
            return struct.pack("<Q", int(value))
        if op == self.OP_EQ_FLOAT or self.OP_LT_FLOAT <= op <= self.OP_GE_FLOAT:
            return struct.pack("<d", float(value))
        if op == self.OP_EQ_BOOL:
            return b"\x01" if value else b"\x00"
        return b""

    def count_where_path(self, path, op, value=None):
        """records whose element at `path` exists and satisfies op (OP_*): value = bytes for OP_EQ_STRING / OP_PREFIX_STRING, an int
        for the *_INT / *_UINT operators, a float for the *_FLOAT ones, a bool for OP_EQ_BOOL"""
        blob, lens, n = self._keys(path)
        v = self._op_value(op, value)
        buf = C.create_string_buffer(v, max(len(v), 1))
        cnt = C.c_uint64(0)
        self._check(_lib.lib().sjhip_count_where_path(self._h, blob, lens, n, int(op), buf, len(v), C.byref(cnt)))
        return cnt.value

    def project_keys(self, keys):
        """Object.ForEach(fn, onlyKeys) (parsed_object.go:142-196) on the root object of every record, on the device.
        -> uint64 array [records, len(keys)]: key number << 56 | tape index of the value of the j-th delivered member,
        2^64 - 1 where there is none"""
        blob, lens, n = self._keys(keys)
        L = _lib.lib()
        cnt = C.c_size_t(0)
        probe = np.empty(1, dtype=np.uint64)
        L.sjhip_project_keys(self._h, blob, lens, n, probe.ctypes.data, 0, C.byref(cnt))  # (no room: only the record count is set)
        out = np.empty((max(cnt.value, 1), n), dtype=np.uint64)
        self._check(L.sjhip_project_keys(self._h, blob, lens, n, out.ctypes.data, out.shape[0], C.byref(cnt)))
        return out[: cnt.value]

    # ---- columns (include/sjhip.h: sjhip_extract_path / _extract_path_strings / _fetch_path_strings) --------------------------
    COL_FLOAT, COL_INT, COL_UINT, COL_BOOL = range(4)
    COL_OK, COL_NOT_FOUND, COL_NOT_OBJECT, COL_TYPE, COL_NULL, COL_RANGE = range(6)
    COL_CVT = 1
    _COL_DTYPES = {0: np.float64, 1: np.int64, 2: np.uint64, 3: np.uint8}

    def extract_path(self, path, kind):
        """Iter.FindElement(path...) then Iter.Float / Int / Uint / Bool (kind = COL_*) on every record, on the device.
        -> (values: float64 / int64 / uint64 / uint8 array, status: uint8 array of COL_OK ... COL_RANGE); 0 where not OK"""
        blob, lens, n = self._keys(path)
        L = _lib.lib()
        dt = self._COL_DTYPES[int(kind)]
        cnt = C.c_size_t(0)
        probe_v, probe_s = np.empty(1, dtype=dt), np.empty(1, dtype=np.uint8)
        L.sjhip_extract_path(self._h, blob, lens, n, int(kind), probe_v.ctypes.data, probe_s.ctypes.data, 0,
                             C.byref(cnt))  # (no room: only the record count is set)
        values = np.empty(max(cnt.value, 1), dtype=dt)
        status = np.empty(max(cnt.value, 1), dtype=np.uint8)
        self._check(L.sjhip_extract_path(self._h, blob, lens, n, int(kind), values.ctypes.data, status.ctypes.data, values.size,
                                         C.byref(cnt)))
        return values[: cnt.value], status[: cnt.value]

    # ---- aggregates (include/sjhip.h: sjhip_aggregate_path / sjhip_aggregate_path_records) ----------------------------------------
    AGG_TILE = 256  # rows per tile of the device's segmented reduction (csrc/query.hip): the shapes of the tests come from it

    def aggregate_path(self, path, kind):
        """count, sum, min and max of the column extract_path(path, kind) returns (kind = COL_FLOAT / COL_INT / COL_UINT), reduced on
        the device over all rows of the selection in force (without one: the records); an empty path: the row's own value.
        -> Aggregate: rows, status (6 ints), count, sum (an exact int, or a float), min, max (None when no row is OK), raw"""
        blob, lens, n = self._keys(path)
        raw = _lib.Agg()
        self._check(_lib.lib().sjhip_aggregate_path(self._h, blob if n else None, lens if n else None, n, int(kind), C.byref(raw)))
        return Aggregate(raw, int(kind))

    def aggregate_path_records(self, path, kind):
        """the same per record: record r reduces the rows fetch_rows gives it (without a selection: its root value).
        -> (count, not_ok: uint64 arrays; sum: float64 array, or the low 64 bits as int64 / uint64; sum_hi: uint64 array -- the
        high 64 bits of an integer sum --; min, max: float64 / int64 / uint64 arrays), one entry per record; a record without an
        OK row has count 0 and zeros"""
        blob, lens, n = self._keys(path)
        L = _lib.lib()
        dt = self._COL_DTYPES[int(kind)]
        cnt = C.c_size_t(0)
        args = (self._h, blob if n else None, lens if n else None, n, int(kind))
        rc = L.sjhip_aggregate_path_records(*args, None, None, None, None, None, None, 0, C.byref(cnt))  # (no room: the record count)
        if rc and not cnt.value:
            self._check(rc)
        m = max(cnt.value, 1)
        count, not_ok, sum_hi = (np.empty(m, dtype=np.uint64) for _ in range(3))  # (the call fills every entry of every record)
        total, lo, hi = (np.empty(m, dtype=dt) for _ in range(3))
        self._check(L.sjhip_aggregate_path_records(*args, count.ctypes.data, not_ok.ctypes.data, total.ctypes.data, sum_hi.ctypes.data,
                                                   lo.ctypes.data, hi.ctypes.data, m, C.byref(cnt)))
        k = cnt.value
        return count[:k], not_ok[:k], total[:k], sum_hi[:k], lo[:k], hi[:k]

    # ---- groups (include/sjhip.h: sjhip_group_path / sjhip_fetch_groups / sjhip_fetch_group_aggregates) --------------------------
    GROUP_NONE, GROUP_NO_VALUE = 0xFFFFFFFF, -1
    GROUP_SORT_TILE = 1024  # rows per tile of the device's sort by code (csrc/sj_sort.h): the largest tile of the grouping's kernels

    def group_path(self, key_path, key_kind, value_path=None, value_kind=None, fetch=True):
        """"group by" on the device: the distinct keys at key_path (key_kind = COL_STRING: Iter.StringBytes, COL_INT: Iter.Int) of the
        rows of the selection in force, in first-occurrence order, a code per row, and -- with value_kind = COL_FLOAT / COL_INT /
        COL_UINT -- count, not_ok, sum, sum_hi, min and max of the column at value_path per key (an empty path: the row's own value).
        -> Groups: rows, groups, key_bytes, keys (a list of bytes, or an int64 array), first_row, group_rows (uint64 arrays), codes
        (uint32, GROUP_NONE where the row has no key), status (uint8, the key's COL_* status) and, when a value was given, the six
        arrays in the shape aggregate_path_records returns; with fetch=False only the three sizes (the grouping stays on the device)"""
        kblob, klens, kn = self._keys(key_path)
        no_value = value_kind is None
        vblob, vlens, vn = self._keys(() if no_value or value_path is None else value_path)
        nr, ng, nb = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_group_path(self._h, kblob if kn else None, klens if kn else None, kn, int(key_kind),
                                                vblob if vn else None, vlens if vn else None, vn,
                                                self.GROUP_NO_VALUE if no_value else int(value_kind), C.byref(nr), C.byref(ng), C.byref(nb)))
        g = Groups(nr.value, ng.value, nb.value, int(key_kind), None if no_value else int(value_kind))
        return self.fetch_groups(g) if fetch else g

    def fetch_groups(self, g):
        """the arrays of the last group_path (g: what it returned with fetch=False) -> g, filled"""
        L = _lib.lib()
        g.first_row, g.group_rows = np.empty(g.groups, dtype=np.uint64), np.empty(g.groups, dtype=np.uint64)
        g.codes, g.status = np.empty(g.rows, dtype=np.uint32), np.empty(g.rows, dtype=np.uint8)
        ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        if g.key_kind == self.COL_INT:
            keys = np.empty(g.groups, dtype=np.int64)
            self._check(L.sjhip_fetch_groups(self._h, None, ptr(keys), ptr(g.first_row), ptr(g.group_rows), ptr(g.codes), ptr(g.status)))
            g.keys, g.key_offsets = keys, None
        else:
            off, data = np.empty(g.groups + 1, dtype=np.uint64), np.empty(g.key_bytes, dtype=np.uint8)
            self._check(L.sjhip_fetch_groups(self._h, off.ctypes.data, ptr(data), ptr(g.first_row), ptr(g.group_rows), ptr(g.codes),
                                             ptr(g.status)))
            raw = data.tobytes()
            g.key_offsets, g.keys = off, [raw[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]
        if g.value_kind is not None:
            dt = self._COL_DTYPES[g.value_kind]
            g.count, g.not_ok, g.sum_hi = (np.empty(g.groups, dtype=np.uint64) for _ in range(3))
            g.sum, g.min, g.max = (np.empty(g.groups, dtype=dt) for _ in range(3))
            self._check(L.sjhip_fetch_group_aggregates(self._h, ptr(g.count), ptr(g.not_ok), ptr(g.sum), ptr(g.sum_hi), ptr(g.min), ptr(g.max)))
        return g

    GROUP_MAX_KEYS, GROUP_MAX_VALUES, GROUP_NULL_KEY = 8, 8, 1  # SJHIP_GROUP_MAX_KEYS, SJHIP_GROUP_MAX_VALUES, SJHIP_GROUP_NULL_KEY

    def group_paths(self, key_columns, value_columns=(), fetch=True):
        """group_path by SEVERAL keys with several aggregates: key_columns = [(path, kind) or (path, kind, null_key), ...], 1 to
        GROUP_MAX_KEYS of them, kind = COL_STRING / COL_INT / COL_UINT / COL_BOOL; value_columns = [(path, kind), ...], up to
        GROUP_MAX_VALUES, kind = COL_FLOAT / COL_INT / COL_UINT.  A row's key is the tuple of its keys; with null_key a row without
        an OK key on that column has the entry "no key" there (such rows tie with each other), without it the row is in no group.
        -> Groups whose key_kind, key_bytes and value_kind are lists (per column) and, after the fetch, so are keys, key_offsets,
        key_ok (uint8 per group: 0 for "no key") and status (uint8 per row); first_row, group_rows and codes are group_path's, and
        values[v] is the tuple (count, not_ok, sum, sum_hi, min, max) of value column v.  fetch=False: only the sizes"""
        kcols = [(tuple(c[0]), int(c[1]), bool(c[2]) if len(c) > 2 else False) for c in key_columns]
        vcols = [(tuple(path), int(kind)) for path, kind in value_columns]
        keys = [bytes(k) for path, *_ in kcols + vcols for k in path]
        nk, nv = len(kcols), len(vcols)
        key_lens = (C.c_uint32 * max(len(keys), 1))(*[len(k) for k in keys])
        kpl = (C.c_uint32 * max(nk, 1))(*[len(path) for path, _, _ in kcols])
        kk = (C.c_int * max(nk, 1))(*[kind for _, kind, _ in kcols])
        kf = (C.c_uint32 * max(nk, 1))(*[self.GROUP_NULL_KEY if nul else 0 for _, _, nul in kcols])
        vpl = (C.c_uint32 * max(nv, 1))(*[len(path) for path, _ in vcols])
        vk = (C.c_int * max(nv, 1))(*[kind for _, kind in vcols])
        nr, ng, nb = C.c_size_t(0), C.c_size_t(0), (C.c_size_t * max(nk, 1))()
        self._check(_lib.lib().sjhip_group_paths(self._h, b"".join(keys) if keys else None, key_lens if keys else None, kpl, kk, kf, nk,
                                                 vpl if nv else None, vk if nv else None, nv, C.byref(nr), C.byref(ng), nb))
        g = Groups(nr.value, ng.value, [int(b) for b in nb[:nk]], [kind for _, kind, _ in kcols], [kind for _, kind in vcols])
        return self.fetch_group_paths(g) if fetch else g

    _GROUP_KEY_DTYPES = {1: np.int64, 2: np.uint64, 3: np.uint8}

    def fetch_group_keys(self, col, kind, groups, key_bytes, rows):
        """column col of the grouping in force (sjhip_fetch_group_keys) -> (keys, key_offsets, key_ok, status): keys a list of bytes
        for COL_STRING, else an int64 / uint64 / uint8 array; key_offsets None but for COL_STRING"""
        ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        key_ok, status = np.empty(groups, dtype=np.uint8), np.empty(rows, dtype=np.uint8)
        if kind == self.COL_STRING:
            off, data = np.empty(groups + 1, dtype=np.uint64), np.empty(key_bytes, dtype=np.uint8)
            self._check(_lib.lib().sjhip_fetch_group_keys(self._h, col, off.ctypes.data, ptr(data), ptr(key_ok), ptr(status)))
            raw = data.tobytes()
            return [raw[int(a):int(b)] for a, b in zip(off[:-1], off[1:])], off, key_ok, status
        keys = np.empty(groups, dtype=self._GROUP_KEY_DTYPES[kind])
        self._check(_lib.lib().sjhip_fetch_group_keys(self._h, col, None, ptr(keys), ptr(key_ok), ptr(status)))
        return keys, None, key_ok, status

    def fetch_group_aggregates_at(self, val, kind, groups):
        """value column val of the grouping in force (sjhip_fetch_group_aggregates_at) -> (count, not_ok, sum, sum_hi, min, max)"""
        ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        dt = self._COL_DTYPES[kind]
        count, not_ok, sum_hi = (np.empty(groups, dtype=np.uint64) for _ in range(3))
        total, lo, hi = (np.empty(groups, dtype=dt) for _ in range(3))
        self._check(_lib.lib().sjhip_fetch_group_aggregates_at(self._h, val, ptr(count), ptr(not_ok), ptr(total), ptr(sum_hi), ptr(lo), ptr(hi)))
        return count, not_ok, total, sum_hi, lo, hi

    def fetch_group_paths(self, g):
        """the arrays of the last group_paths (g: what it returned with fetch=False) -> g, filled"""
        ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        g.first_row, g.group_rows = np.empty(g.groups, dtype=np.uint64), np.empty(g.groups, dtype=np.uint64)
        g.codes = np.empty(g.rows, dtype=np.uint32)
        self._check(_lib.lib().sjhip_fetch_groups(self._h, None, None, ptr(g.first_row), ptr(g.group_rows), ptr(g.codes), None))
        g.keys, g.key_offsets, g.key_ok, g.status = [], [], [], []
        for col, (kind, nbytes) in enumerate(zip(g.key_kind, g.key_bytes)):
            for dst, a in zip((g.keys, g.key_offsets, g.key_ok, g.status), self.fetch_group_keys(col, kind, g.groups, nbytes, g.rows)):
                dst.append(a)
        g.values = [self.fetch_group_aggregates_at(v, kind, g.groups) for v, kind in enumerate(g.value_kind)]
        return g

    def extract_path_strings(self, path, cvt=False, fetch=True):
        """Iter.FindElement(path...) then Iter.StringBytes (or StringCvt with cvt=True) on every record, built on the device.
        -> (offsets: uint64 array of records + 1, data: bytes, status: uint8 array) -- Arrow's large-string layout; with
        fetch=False the column stays on the device and (records, bytes) is returned"""
        blob, lens, n = self._keys(path)
        L = _lib.lib()
        nr, nb = C.c_size_t(0), C.c_size_t(0)
        self._check(L.sjhip_extract_path_strings(self._h, blob, lens, n, self.COL_CVT if cvt else 0, C.byref(nr), C.byref(nb)))
        if not fetch:
            return nr.value, nb.value
        return self.fetch_path_strings(nr.value, nb.value)

    def fetch_path_strings(self, records, nbytes):
        """the column of the last extract_path_strings (its records and bytes) -> (offsets, data, status)"""
        offsets = np.empty(records + 1, dtype=np.uint64)
        data = np.empty(max(nbytes, 1), dtype=np.uint8)
        status = np.empty(max(records, 1), dtype=np.uint8)
        self._check(_lib.lib().sjhip_fetch_path_strings(self._h, offsets.ctypes.data, data.ctypes.data, status.ctypes.data))
        return offsets, data[:nbytes].tobytes(), status[:records]

    # ---- list columns (include/sjhip.h: sjhip_extract_path_list / _list_strings and their fetches) -----------------------------
    def extract_path_list(self, path, kind, fetch=True):
        """Iter.FindElement(path...), Iter.Array, then Array.AsFloat / AsInteger / AsUint64 (kind = COL_FLOAT / COL_INT / COL_UINT)
        on every record, on the device.  -> (list_offsets: uint64 array of records + 1, values: float64 / int64 / uint64 array,
        status: uint8 array) -- Arrow's large_list layout; with fetch=False the column stays on the device and
        (records, elems) is returned"""
        blob, lens, n = self._keys(path)
        nr, ne = C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_extract_path_list(self._h, blob, lens, n, int(kind), C.byref(nr), C.byref(ne)))
        if not fetch:
            return nr.value, ne.value
        return self.fetch_path_list(nr.value, ne.value, kind)

    def fetch_path_list(self, records, elems, kind):
        """the column of the last extract_path_list (its records, elements and kind) -> (list_offsets, values, status)"""
        offsets = np.empty(records + 1, dtype=np.uint64)
        values = np.empty(max(elems, 1), dtype=self._COL_DTYPES[int(kind)])
        status = np.empty(max(records, 1), dtype=np.uint8)
        self._check(_lib.lib().sjhip_fetch_path_list(self._h, offsets.ctypes.data, values.ctypes.data, status.ctypes.data))
        return offsets, values[:elems], status[:records]

    def extract_path_list_strings(self, path, cvt=False, fetch=True):
        """... then Array.AsString (or AsStringCvt with cvt=True).  -> (list_offsets: uint64 array of records + 1, str_offsets:
        uint64 array of elems + 1, data: bytes, status: uint8 array) -- Arrow's large_list<large_string>; with fetch=False
        the column stays on the device and (records, elems, bytes) is returned"""
        blob, lens, n = self._keys(path)
        nr, ne, nb = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_extract_path_list_strings(self._h, blob, lens, n, self.COL_CVT if cvt else 0, C.byref(nr),
                                                               C.byref(ne), C.byref(nb)))
        if not fetch:
            return nr.value, ne.value, nb.value
        return self.fetch_path_list_strings(nr.value, ne.value, nb.value)

    def fetch_path_list_strings(self, records, elems, nbytes):
        """the column of the last extract_path_list_strings -> (list_offsets, str_offsets, data, status)"""
        offsets = np.empty(records + 1, dtype=np.uint64)
        soff = np.empty(elems + 1, dtype=np.uint64)
        data = np.empty(max(nbytes, 1), dtype=np.uint8)
        status = np.empty(max(records, 1), dtype=np.uint8)
        self._check(_lib.lib().sjhip_fetch_path_list_strings(self._h, offsets.ctypes.data, soff.ctypes.data, data.ctypes.data,
                                                             status.ctypes.data))
        return offsets, soff, data[:nbytes].tobytes(), status[:records]

    # ---- tables (include/sjhip.h: sjhip_extract_table / sjhip_fetch_table_column) -----------------------------------------------
    COL_STRING, COL_STRING_CVT = 4, 5  # kinds of table columns only: Iter.StringBytes / Iter.StringCvt
    TABLE_MAX_COLS = 16

    def extract_table(self, columns, fetch=True):
        """columns: a list of (path, kind), kind = COL_FLOAT / INT / UINT / BOOL / COL_STRING / COL_STRING_CVT -- all of them
        evaluated in one walk of every record, on the device.  -> one entry per column, shaped like extract_path's
        (values, status) or extract_path_strings' (offsets, data, status); with fetch=False the table stays on the device and
        (records, [text bytes of every column]) is returned (fetch_table_column)"""
        keys = [bytes(k) for path, _ in columns for k in path]
        n = len(columns)
        key_lens = (C.c_uint32 * max(len(keys), 1))(*[len(k) for k in keys])
        path_lens = (C.c_uint32 * max(n, 1))(*[len(path) for path, _ in columns])
        kinds = (C.c_int * max(n, 1))(*[int(kind) for _, kind in columns])
        nr, nb = C.c_size_t(0), (C.c_size_t * max(n, 1))()
        self._check(_lib.lib().sjhip_extract_table(self._h, b"".join(keys), key_lens, path_lens, kinds, n, C.byref(nr), nb))
        sizes = [int(b) for b in nb[:n]]
        if not fetch:
            return nr.value, sizes
        return [self.fetch_table_column(c, nr.value, kind, sizes[c]) for c, (_, kind) in enumerate(columns)]

    def fetch_table_column(self, col, records, kind, nbytes=0):
        """column `col` of the last extract_table (the table's records, the column's kind and text bytes) -> (values, status)
        or (offsets, data, status)"""
        L = _lib.lib()
        status = np.empty(max(records, 1), dtype=np.uint8)
        if int(kind) in (self.COL_STRING, self.COL_STRING_CVT):
            offsets = np.empty(records + 1, dtype=np.uint64)
            data = np.empty(max(nbytes, 1), dtype=np.uint8)
            self._check(L.sjhip_fetch_table_column(self._h, int(col), None, offsets.ctypes.data, data.ctypes.data, status.ctypes.data))
            return offsets, data[:nbytes].tobytes(), status[:records]
        values = np.empty(max(records, 1), dtype=self._COL_DTYPES[int(kind)])
        self._check(L.sjhip_fetch_table_column(self._h, int(col), values.ctypes.data, None, None, status.ctypes.data))
        return values[:records], status[:records]

    # ---- rows (include/sjhip.h: sjhip_select_rows / sjhip_fetch_rows / sjhip_select_records) -----------------------------------
    def select_rows(self, path=()):
        """Iter.FindElement(path...), Iter.Array, Array.Iter on every record: the elements of that array become the rows, and the
        path queries, columns, lists and tables above run on every row until select_records() or the next parse.  An empty path:
        the array is the record's root value.  -> (records, rows)"""
        blob, lens, n = self._keys(path)
        nr, nw = C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_select_rows(self._h, blob if n else None, lens if n else None, n, C.byref(nr), C.byref(nw)))
        return nr.value, nw.value

    def fetch_rows(self, records, rows):
        """the selection of the last select_rows (its records and rows) -> (row_offsets: uint64 array of records + 1, row_index:
        uint64 array of the tape index of every row's value, status: uint8 array of COL_OK ... per record)"""
        offsets = np.empty(records + 1, dtype=np.uint64)
        index = np.empty(max(rows, 1), dtype=np.uint64)
        status = np.empty(max(records, 1), dtype=np.uint8)
        self._check(_lib.lib().sjhip_fetch_rows(self._h, offsets.ctypes.data, index.ctypes.data, status.ctypes.data))
        return offsets, index[:rows], status[:records]

    def select_records(self):
        """back to one row per record (no error if nothing was selected)"""
        self._check(_lib.lib().sjhip_select_records(self._h))

    def where_path(self, path, op, value=None, negate=False):
        """keeps the rows -- of the selection in force, or without one the records, which then become a selection of one row each --
        whose element at `path` exists and satisfies op (count_where_path's predicate and values; an empty path: the row's own
        value); negate: keeps the others instead.  Successive calls narrow further; select_records() goes back.
        -> (records, rows kept); fetch_rows(records, rows) delivers the selection"""
        blob, lens, n = self._keys(path)
        v = self._op_value(op, value)
        buf = C.create_string_buffer(v, max(len(v), 1))
        nr, nw = C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_where_path(self._h, blob if n else None, lens if n else None, n, int(op), buf, len(v),
                                                self.WHERE_NOT if negate else 0, C.byref(nr), C.byref(nw)))
        return nr.value, nw.value

    WHERE_AND, WHERE_OR, WHERE_NEG = 0x80, 0x81, 0x82  # SJHIP_WHERE_AND / _OR / _NEG: the operators of a program
    WHERE_MAX_PREDS = 16     # SJHIP_WHERE_MAX_PREDS
    WHERE_MAX_PROGRAM = 64   # SJHIP_WHERE_MAX_PROGRAM

    def _where_paths_args(self, predicates, program):
        preds = [(tuple(path), int(op), self._op_value(int(op), value)) for path, op, value in predicates]
        keys = [bytes(k) for path, _, _ in preds for k in path]
        n = len(preds)
        key_lens = (C.c_uint32 * max(len(keys), 1))(*[len(k) for k in keys])
        path_lens = (C.c_uint32 * max(n, 1))(*[len(path) for path, _, _ in preds])
        ops = (C.c_int * max(n, 1))(*[op for _, op, _ in preds])
        values = b"".join(v for _, _, v in preds)
        value_lens = (C.c_uint32 * max(n, 1))(*[len(v) for _, _, v in preds])
        program = bytes(program)
        return (self._h, b"".join(keys) if keys else None, key_lens if keys else None, path_lens, ops,
                C.create_string_buffer(values, max(len(values), 1)), value_lens, n, program, len(program))

    def where_paths(self, predicates, program):
        """where_path for SEVERAL tests from one walk of every row: predicates = [(path, op, value), ...], 1 to WHERE_MAX_PREDS of
        them, each where_path's predicate (an empty path: the row's own value); program = bytes, postfix: a byte p < len(predicates)
        pushes the truth of predicate p, WHERE_AND / WHERE_OR pop two values and push one, WHERE_NEG replaces the top -- e.g.
        bytes([0, 1, WHERE_OR]) for "a in (x, y)".  Every predicate must be named, one value must be left.  Keeps the rows for
        which the program is true; narrowing and composition are where_path's.  -> (records, rows kept)"""
        nr, nw = C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_where_paths(*self._where_paths_args(predicates, program), C.byref(nr), C.byref(nw)))
        return nr.value, nw.value

    def count_where_paths(self, predicates, program):
        """the rows where_paths(predicates, program) would keep; the selection stays as it is"""
        cnt = C.c_uint64(0)
        self._check(_lib.lib().sjhip_count_where_paths(*self._where_paths_args(predicates, program), C.byref(cnt)))
        return cnt.value

    WHERE_IN_MAX_VALUES = 1 << 24  # SJHIP_WHERE_IN_MAX_VALUES

    def _where_in_args(self, path, kind, values, negate):
        """the arguments of sjhip_where_path_in up to `flags`, and the arrays they point into (to be kept until the call returns)"""
        blob, lens, n = self._keys(path)
        kind = int(kind)
        offs = data = None
        if kind == self.COL_STRING:
            if isinstance(values, tuple) and len(values) == 2 and isinstance(values[0], np.ndarray):
                offs = np.ascontiguousarray(values[0], dtype=np.uint64)
                data = np.ascontiguousarray(values[1], dtype=np.uint8)
            else:
                vs = [bytes(v) for v in values]
                offs = np.zeros(len(vs) + 1, dtype=np.uint64)
                offs[1:] = np.cumsum([len(v) for v in vs], dtype=np.uint64)
                data = np.frombuffer(b"".join(vs), dtype=np.uint8)
            count = max(len(offs) - 1, 0)
        elif isinstance(values, np.ndarray) and values.dtype in (np.int64, np.uint64):
            data, count = np.ascontiguousarray(values), len(values)
        else:
            data = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in values], dtype=np.uint64)
            count = len(data)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        args = (self._h, blob if n else None, lens if n else None, n, kind, ptr(offs) if count else None, ptr(data), count,
                self.WHERE_NOT if negate else 0)
        return args, (offs, data)

    def where_path_in(self, path, kind, values, negate=False):
        """where_path by MEMBERSHIP: keeps the rows whose element at `path` (an empty path: the row's own value) equals one of
        `values` as OP_EQ_STRING (kind = COL_STRING), OP_EQ_INT (COL_INT) or OP_EQ_UINT (COL_UINT) compare -- a list of bytes, or
        an (offsets, data) pair of numpy arrays in Arrow's large-string layout; a list or an int64 / uint64 array of ints.  What
        group_path returns as keys can be passed straight back.  negate: keeps the others instead, the rows without a usable key
        included.  Duplicates change nothing; no values: no row matches.  Narrowing and composition are where_path's.
        -> (records, rows kept)"""
        args, keep = self._where_in_args(path, kind, values, negate)
        nr, nw = C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_where_path_in(*args, C.byref(nr), C.byref(nw)))
        del keep
        return nr.value, nw.value

    def count_where_path_in(self, path, kind, values, negate=False):
        """the rows where_path_in(path, kind, values, negate) would keep; the selection stays as it is"""
        args, keep = self._where_in_args(path, kind, values, negate)
        cnt = C.c_uint64(0)
        self._check(_lib.lib().sjhip_count_where_path_in(*args, C.byref(cnt)))
        del keep
        return cnt.value

    # ---- unnest (include/sjhip.h: sjhip_unnest_rows / sjhip_fetch_row_parents) ---------------------------------------------------
    def unnest_rows(self, path=()):
        """Iter.FindElement(path...), Iter.Array, Array.Iter on every ROW of the selection in force (without one: on every record's
        root value): the elements of those arrays become the rows, every record keeps its status byte and owns the new rows that
        came from the rows it owned.  An empty path: the row's own value is the array (lists of lists).
        -> (records, parents: the rows before the call, rows: the rows after it); fetch_rows(records, rows) delivers the
        selection, fetch_row_parents(parents, rows) the join back"""
        blob, lens, n = self._keys(path)
        nr, npar, nw = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_unnest_rows(self._h, blob if n else None, lens if n else None, n, C.byref(nr), C.byref(npar),
                                                 C.byref(nw)))
        return nr.value, npar.value, nw.value

    def fetch_row_parents(self, parents, rows):
        """the join back of the last unnest_rows (its parents and rows) -> (parent_offsets: uint64 array of parents + 1 over the new
        rows, parent: uint64 array of the parent row number of every new row -- what np.take needs to repeat a parent column
        fetched before the call --, parent_status: uint8 array of COL_OK ... per parent).  Parent numbers count in the selection
        as it was before the call, row numbers in the one the call left"""
        offsets = np.empty(parents + 1, dtype=np.uint64)
        parent = np.empty(max(rows, 1), dtype=np.uint64)
        status = np.empty(max(parents, 1), dtype=np.uint8)
        self._check(_lib.lib().sjhip_fetch_row_parents(self._h, offsets.ctypes.data, parent.ctypes.data, status.ctypes.data))
        return offsets, parent[:rows], status[:parents]

    # ---- member rows (include/sjhip.h: sjhip_unnest_members / sjhip_extract_row_names / sjhip_where_row_names) ----------------------
    def unnest_members(self, path=()):
        """Iter.FindElement(path...), Iter.Object, Object.ForEach on every ROW of the selection in force (without one: on every
        record's root value): the VALUES of the members of those objects become the rows, duplicate names included; unnest_rows'
        contract otherwise.  An empty path: the row's own value is the object (maps of maps).
        -> (records, parents, rows); fetch_rows and fetch_row_parents deliver the selection and the join back,
        extract_row_names the names"""
        blob, lens, n = self._keys(path)
        nr, npar, nw = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_unnest_members(self._h, blob if n else None, lens if n else None, n, C.byref(nr), C.byref(npar),
                                                    C.byref(nw)))
        return nr.value, npar.value, nw.value

    def extract_row_names(self, fetch=True):
        """the unescaped member names of the rows in force -- unnest_members' rows, or what where_* / order_*(limit) kept of them --
        as the string column.  -> extract_path_strings' (offsets, data, status), every status COL_OK; with fetch=False the column
        stays on the device and (rows, bytes) is returned (fetch_path_strings delivers it)"""
        nr, nb = C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_extract_row_names(self._h, C.byref(nr), C.byref(nb)))
        if not fetch:
            return nr.value, nb.value
        return self.fetch_path_strings(nr.value, nb.value)

    def where_row_names(self, op, value, negate=False):
        """where_path with the row's member name in the place of the element at a path: op = OP_EQ_STRING or OP_PREFIX_STRING,
        value = bytes; negate keeps the others.  Needs a selection of members.  -> (records, rows kept)"""
        v = bytes(value)
        buf = C.create_string_buffer(v, max(len(v), 1))
        nr, nw = C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_where_row_names(self._h, int(op), buf, len(v), self.WHERE_NOT if negate else 0, C.byref(nr),
                                                     C.byref(nw)))
        return nr.value, nw.value

    # ---- row schema (include/sjhip.h: sjhip_row_schema / sjhip_fetch_row_schema) -------------------------------------------------
    TYPE_NULL, TYPE_STRING, TYPE_INT, TYPE_UINT, TYPE_FLOAT, TYPE_BOOL, TYPE_OBJECT, TYPE_ARRAY = range(1, 9)  # SJHIP_TYPE_*
    SCHEMA_TYPES = 8  # SJHIP_SCHEMA_TYPES

    def row_schema(self, path=(), fetch=True):
        """Iter.FindElement(path...), Iter.Object on every ROW of the selection in force (without one: on every record's root value)
        and the direct members of those objects counted by (unescaped name, type of the value); the selection and every other
        product stay as they are.  An empty path: the row's own value is the object.
        -> Schema: rows, status (uint64 array of 6: the rows per COL_* status), members, n_names, name_bytes and -- unless fetch=False,
        when the schema stays on the device for fetch_row_schema -- names (a list of bytes, in first-occurrence order), first_row
        (uint64 array: the first row that has the name) and counts (uint64 array [names, 8]: column TYPE_x - 1 counts the members
        of that name whose value has type x)"""
        blob, lens, n = self._keys(path)
        status = (C.c_uint64 * 6)()
        nr, nn, nb, nm = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        self._check(_lib.lib().sjhip_row_schema(self._h, blob if n else None, lens if n else None, n, C.byref(nr), status, C.byref(nm),
                                                C.byref(nn), C.byref(nb)))
        s = Schema(nr.value, np.array(list(status), dtype=np.uint64), nm.value, nn.value, nb.value)
        return self.fetch_row_schema(s) if fetch else s

    def fetch_row_schema(self, s):
        """the arrays of the last row_schema (s: what it returned with fetch=False) -> s, filled"""
        off, data = np.empty(s.n_names + 1, dtype=np.uint64), np.empty(max(s.name_bytes, 1), dtype=np.uint8)
        s.first_row = np.empty(s.n_names, dtype=np.uint64)
        s.counts = np.empty((s.n_names, self.SCHEMA_TYPES), dtype=np.uint64)
        ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        self._check(_lib.lib().sjhip_fetch_row_schema(self._h, off.ctypes.data, data.ctypes.data, ptr(s.first_row), ptr(s.counts)))
        raw = data.tobytes()
        s.name_offsets, s.names = off, [raw[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]
        return s

    # ---- order (include/sjhip.h: sjhip_order_path / sjhip_fetch_order) -----------------------------------------------------------
    ORDER_DESC = 1
    ORDER_SORT_TILE = 1024  # rows per tile of the device's sort by key (csrc/sj_sort.h): the largest tile of the ordering's kernels

    def order_path(self, path, kind, descending=False, limit=0, fetch=True):
        """"order by ... limit k" on the device: ranks the rows of the selection in force (without one: the records) by the element
        at `path` converted by kind = COL_FLOAT / COL_INT / COL_UINT (an empty path: the row's own value) -- OK rows first, ascending
        or descending by key, equal keys in row order, the rows without an OK key last in row order -- and narrows the selection, as
        where_path would, to the rows of rank < limit (0: all).  The selection stays in document order.
        -> Order: records, rows (the rows kept), kind and, fetched, order (uint64: order[i] is the row number in the narrowed
        selection of the row of rank i), values (float64 / int64 / uint64, in rank order, 0 where not OK) and status (uint8); with
        fetch=False only the sizes (the order stays on the device: fetch_order)"""
        blob, lens, n = self._keys(path)
        nr, nw = C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_order_path(self._h, blob if n else None, lens if n else None, n, int(kind),
                                                self.ORDER_DESC if descending else 0, int(limit), C.byref(nr), C.byref(nw)))
        o = Order(nr.value, nw.value, int(kind))
        return self.fetch_order(o) if fetch else o

    def order_path_strings(self, path, descending=False, limit=0, fetch=True):
        """order_path by a STRING key: the element at `path` as Iter.StringBytes returns it (an empty path: the row's own value) --
        the rows with a string first, ascending or descending by their unescaped bytes compared as unsigned bytes, a proper prefix in
        front of the longer key (code point order for UTF-8, not a collation); equal keys in row order, the rows without a string
        last in row order.  Limit, narrowing and composition are order_path's.
        -> Order with kind = COL_STRING and values = None: the sorted keys are extract_path_strings on the kept rows taken through
        `order`"""
        blob, lens, n = self._keys(path)
        nr, nw = C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_order_path_strings(self._h, blob if n else None, lens if n else None, n,
                                                        self.ORDER_DESC if descending else 0, int(limit), C.byref(nr), C.byref(nw)))
        o = Order(nr.value, nw.value, self.COL_STRING)
        return self.fetch_order(o) if fetch else o

    ORDER_MAX_KEYS = 8  # SJHIP_ORDER_MAX_KEYS
    ORDER_MULTI = -1    # Order.kind of an order by several keys (it has no values)

    def order_paths(self, columns, limit=0, fetch=True):
        """order_path by SEVERAL keys: columns = [(path, kind, descending), ...], 1 to ORDER_MAX_KEYS of them, kind = COL_FLOAT /
        COL_INT / COL_UINT (order_path's key and status) or COL_STRING (order_path_strings'), each ascending or descending.  The
        order is the one a stable sort by the tuple gives: rows that tie on column 0 -- the rows without an OK key there tie with
        each other, behind the others -- are compared on column 1, and so on; rows that tie everywhere stay in row order.  The
        limit is applied once, at the end; narrowing and composition are order_path's.
        -> Order with kind = ORDER_MULTI and values = None; status is the status on column 0.  The sorted keys are extract_table on
        the kept rows taken through `order`"""
        cols = [(tuple(path), int(kind), bool(desc)) for path, kind, desc in columns]
        keys = [bytes(k) for path, _, _ in cols for k in path]
        n = len(cols)
        key_lens = (C.c_uint32 * max(len(keys), 1))(*[len(k) for k in keys])
        path_lens = (C.c_uint32 * max(n, 1))(*[len(path) for path, _, _ in cols])
        kinds = (C.c_int * max(n, 1))(*[kind for _, kind, _ in cols])
        flags = (C.c_uint32 * max(n, 1))(*[self.ORDER_DESC if desc else 0 for _, _, desc in cols])
        nr, nw = C.c_size_t(0), C.c_size_t(0)
        self._check(_lib.lib().sjhip_order_paths(self._h, b"".join(keys) if keys else None, key_lens if keys else None, path_lens, kinds,
                                                 flags, n, int(limit), C.byref(nr), C.byref(nw)))
        o = Order(nr.value, nw.value, self.ORDER_MULTI)
        return self.fetch_order(o) if fetch else o

    def fetch_order(self, o):
        """the arrays of the last order_path / order_path_strings / order_paths (o: what it returned with fetch=False) -> o, filled
        (a string order and an order by several keys have no values: None)"""
        o.order, o.status = np.empty(o.rows, dtype=np.uint64), np.empty(o.rows, dtype=np.uint8)
        o.values = None if o.kind in (self.COL_STRING, self.ORDER_MULTI) else np.empty(o.rows, dtype=self._COL_DTYPES[o.kind])
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        self._check(_lib.lib().sjhip_fetch_order(self._h, ptr(o.order), ptr(o.values), ptr(o.status)))
        return o

    def filter_rows(self, fetch=True):
        """The rows of the selection in force (select_rows / where_path) as a new self-contained (Tape, Strings.B) on the device,
        one root per row -- what ParseND returns for the document whose lines are the texts of those rows; scalar rows are left
        out and counted.  where_path + filter_rows is filter_where for every operator, conjunctions, nested paths and rows inside
        arrays.  -> (n_rows, skipped, ParsedJson), or with fetch=False (n_rows, skipped, (tape_len, strings_len)) and the result
        stays on the device"""
        n, sk, tl, sl = C.c_uint64(0), C.c_uint64(0), C.c_size_t(0), C.c_size_t(0)
        L = _lib.lib()
        self._check(L.sjhip_filter_rows(self._h, C.byref(n), C.byref(sk), C.byref(tl), C.byref(sl)))
        if not fetch:
            return n.value, sk.value, (tl.value, sl.value)
        tape = np.empty(tl.value, dtype=np.uint64)
        strings = np.empty(sl.value, dtype=np.uint8)
        self._check(L.sjhip_fetch_filtered(self._h, tape.ctypes.data, strings.ctypes.data))
        return n.value, sk.value, ParsedJson(b"", tape, strings)

    def serialize(self, fetch=True, dedup=False):
        """Serializer.Serialize (format v3, CompressNone) of the device-resident result of the last parse.
        -> the framed stream as a uint8 array (what the reference's Deserialize reads), or its sizes with fetch=False.
        dedup: de-duplicate the strings like the reference's indexString (the plain form is byte-identical to the
        oracle's stream without de-duplication)."""
        L = _lib.lib()
        tl, vl, sl, n = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(L.sjhip_serialize_ex(self._h, 1 if dedup else 0, C.byref(tl), C.byref(vl), C.byref(sl), C.byref(n)))
        if not fetch:
            return {"tags": tl.value, "values": vl.value, "strings": sl.value, "stream": n.value}
        out = np.empty(n.value, dtype=np.uint8)
        got = C.c_size_t(0)
        self._check(L.sjhip_fetch_serialized(self._h, out.ctypes.data, out.size, C.byref(got)))
        return out[: got.value]

    def deserialize(self, stream):
        """Serializer.Deserialize of a stream with uncompressed blocks, on the device -> ParsedJson (strings point into
        Message = the string column, like the reference's result)."""
        L = _lib.lib()
        a = np.frombuffer(stream, dtype=np.uint8) if not isinstance(stream, np.ndarray) else stream
        tl, sl, ml = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(L.sjhip_deserialize(self._h, a.ctypes.data, a.size, C.byref(tl), C.byref(sl), C.byref(ml)))
        tape, strings = self.fetch(tl.value, sl.value)
        msg = np.empty(ml.value, dtype=np.uint8)
        self._check(L.sjhip_fetch_message(self._h, msg.ctypes.data))
        return ParsedJson(msg.tobytes(), tape, strings)

    def marshal_json(self, fetch=True):
        """pj.Iter().MarshalJSON() of the device-resident result of the last parse: compact JSON text, records
        separated by newlines.  -> bytes (or the length with fetch=False)"""
        L = _lib.lib()
        n = C.c_size_t(0)
        self._check(L.sjhip_marshal_json(self._h, C.byref(n)))
        if not fetch:
            return n.value
        out = np.empty(n.value, dtype=np.uint8)
        self._check(L.sjhip_fetch_marshaled(self._h, out.ctypes.data))
        return out.tobytes()

    def marshal_rows(self, fetch=True, offsets=False):
        """The rows of the selection in force (select_rows / where_path) as NDJSON text built on the device: the compact JSON text
        of every row, in selection order, joined by newlines (none behind the last); a scalar row is its own text.
        -> (n_rows, text) or, with offsets=True, (n_rows, text, offsets): a uint64 array of n_rows + 1 entries, row i is
        text[offsets[i]:offsets[i + 1] - 1]; with fetch=False (n_rows, text_len) and the text stays on the device"""
        L = _lib.lib()
        n, tl = C.c_uint64(0), C.c_size_t(0)
        self._check(L.sjhip_marshal_rows(self._h, C.byref(n), C.byref(tl)))
        if not fetch:
            return n.value, tl.value
        out = np.empty(tl.value, dtype=np.uint8)
        off = np.empty(n.value + 1, dtype=np.uint64) if offsets else None
        self._check(L.sjhip_fetch_marshaled_rows(self._h, off.ctypes.data if offsets else None, out.ctypes.data))
        return (n.value, out.tobytes(), off) if offsets else (n.value, out.tobytes())

    PROJECT_NULLS = 1

    def marshal_rows_paths(self, columns, names=None, nulls=False, fetch=True, offsets=False):
        """marshal_rows with a select list: of every row of the selection in force only the elements at the paths of `columns` (1 to
        16 paths, each a sequence of keys; an empty path: the row's own value), as one JSON object per row.  names: the member name
        of every column (bytes; None: the last key of its path).  A column whose path is not found in a row is left out of that
        row, or written as null with nulls=True.  -> what marshal_rows returns"""
        L = _lib.lib()
        keys = [bytes(k) for path in columns for k in path]
        nc = len(columns)
        key_lens = (C.c_uint32 * max(len(keys), 1))(*[len(k) for k in keys])
        path_lens = (C.c_uint32 * max(nc, 1))(*[len(path) for path in columns])
        blob = name_lens = None
        if names is not None:
            ns = [bytes(x) for x in names]
            if len(ns) != nc:
                raise ValueError("marshal_rows_paths: %d names for %d columns" % (len(ns), nc))
            blob, name_lens = b"".join(ns), (C.c_uint32 * max(nc, 1))(*[len(x) for x in ns])
        n, tl = C.c_uint64(0), C.c_size_t(0)
        self._check(L.sjhip_marshal_rows_paths(self._h, b"".join(keys), key_lens, path_lens, nc, blob, name_lens,
                                               self.PROJECT_NULLS if nulls else 0, C.byref(n), C.byref(tl)))
        if not fetch:
            return n.value, tl.value
        out = np.empty(tl.value, dtype=np.uint8)
        off = np.empty(n.value + 1, dtype=np.uint64) if offsets else None
        self._check(L.sjhip_fetch_marshaled_rows(self._h, off.ctypes.data if offsets else None, out.ctypes.data))
        return (n.value, out.tobytes(), off) if offsets else (n.value, out.tobytes())

    def fetch(self, tape_len, strings_len):
        tape = np.empty(tape_len, dtype=np.uint64)
        strings = np.empty(strings_len, dtype=np.uint8)
        self._check(_lib.lib().sjhip_fetch(self._h, tape.ctypes.data, strings.ctypes.data))
        return tape, strings


class Aggregate:
    """what Context.aggregate_path returns: the sjhip_agg of the call (raw) read for its kind"""

    def __init__(self, raw, kind):
        import struct
        self.raw, self.kind = raw, kind
        self.rows = int(raw.rows)
        self.status = [int(x) for x in raw.status]
        self.count = self.status[Context.COL_OK]
        fmt = {Context.COL_FLOAT: "<d", Context.COL_INT: "<q", Context.COL_UINT: "<Q"}[kind]
        value = lambda bits: struct.unpack(fmt, struct.pack("<Q", int(bits)))[0]  # noqa: E731
        if kind == Context.COL_FLOAT:
            self.sum = value(raw.sum_lo)
        else:
            self.sum = (int(raw.sum_hi) << 64) | int(raw.sum_lo)
            if kind == Context.COL_INT and self.sum >> 127:
                self.sum -= 1 << 128
        self.min = value(raw.min) if self.count else None
        self.max = value(raw.max) if self.count else None

    def __repr__(self):
        return f"Aggregate(rows={self.rows}, status={self.status}, sum={self.sum!r}, min={self.min!r}, max={self.max!r})"


class Groups:
    """what Context.group_path returns: the sizes of the grouping, and after the fetch its arrays (see group_path); from
    Context.group_paths key_bytes, key_kind and value_kind are lists with one entry per column, and so are the fetched keys,
    key_offsets, key_ok, status and values (see group_paths)"""

    def __init__(self, rows, groups, key_bytes, key_kind, value_kind):
        self.rows, self.groups, self.key_bytes, self.key_kind, self.value_kind = rows, groups, key_bytes, key_kind, value_kind

    def aggregates(self):
        """(count, not_ok, sum, sum_hi, min, max): the tuple aggregate_path_records returns, per group"""
        return self.count, self.not_ok, self.sum, self.sum_hi, self.min, self.max

    def __repr__(self):
        return f"Groups(rows={self.rows}, groups={self.groups}, key_bytes={self.key_bytes})"


class Schema:
    """what Context.row_schema returns: rows, status, members, n_names and name_bytes, and after the fetch names, name_offsets,
    first_row and counts (see row_schema)"""

    def __init__(self, rows, status, members, n_names, name_bytes):
        self.rows, self.status, self.members, self.n_names, self.name_bytes = rows, status, members, n_names, name_bytes
        self.names = self.name_offsets = self.first_row = self.counts = None

    def __repr__(self):
        return f"Schema(rows={self.rows}, members={self.members}, names={self.n_names}, name_bytes={self.name_bytes})"


class Order:
    """what Context.order_path / order_path_strings / order_paths return: the records, the rows kept and the kind of the keys
    (Context.ORDER_MULTI after order_paths), and after the fetch order, values (None for a string order and for an order by
    several keys) and status (after order_paths: the status on column 0) in rank order (see order_path)"""

    def __init__(self, records, rows, kind):
        self.records, self.rows, self.kind = records, rows, kind

    def __repr__(self):
        return f"Order(records={self.records}, rows={self.rows}, kind={self.kind})"


class MultiContext:
    """ParseND over several GPUs in one call (include/sjhip.h: sjhip_multi_*): one shard per entry of `devices`
    (None = every visible device; a device may be listed more than once)."""

    def __init__(self, devices=None):
        L = _lib.lib()
        if devices is None:
            self._h = L.sjhip_multi_create(None, 0)
        else:
            arr = (C.c_int * len(devices))(*devices)
            self._h = L.sjhip_multi_create(arr, len(devices))
        if not self._h:
            raise ParseError(ERR_NODEVICE, 3)
        self.shards = L.sjhip_multi_shards(self._h)

    def close(self):
        if self._h:
            _lib.lib().sjhip_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def parse_nd(self, data, copy_strings=True):
        """ParseND(data): the merged ParsedJson of all shards (bit for bit what one context returns)."""
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        tl, sl, mo, ml = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        L = _lib.lib()
        rc = L.sjhip_parse_nd_multi(self._h, a.ctypes.data if a.size else None, a.size, FLAG_NDJSON | (FLAG_COPY_STRINGS if copy_strings else 0),
                                    C.byref(tl), C.byref(sl), C.byref(mo), C.byref(ml))
        if rc == 1:
            raise ParseError(ERR_STAGE1, rc)
        if rc == 2:
            raise ParseError(ERR_STAGE2, rc)
        if rc:
            raise ParseError(f"sjhip error {rc}: {L.sjhip_multi_last_error(self._h).decode()}", rc)
        tape = np.empty(tl.value, dtype=np.uint64)
        strings = np.empty(sl.value, dtype=np.uint8)
        rc = L.sjhip_fetch_multi(self._h, tape.ctypes.data, strings.ctypes.data)
        if rc:
            raise ParseError(f"sjhip error {rc}: {L.sjhip_multi_last_error(self._h).decode()}", rc)
        return ParsedJson(a[mo.value: mo.value + ml.value].tobytes(), tape, strings)


class ParsedJson:
    """parsed_json.go:64-71: Message / Tape / Strings."""

    __slots__ = ("_msg", "Tape", "Strings", "_tape_buf", "_str_buf", "records", "device", "_owner")

    def __init__(self, message, tape, strings, tape_buf=None, str_buf=None):
        # `message`: bytes, or a uint8 view of the caller's buffer -- the reference's pj.Message ALIASES the input
        # (bytes.TrimSpace, parse_json_amd64.go:55); the bytes object is only made when somebody asks for it
        self._msg = message
        self.Tape = tape
        self.Strings = strings
        self._tape_buf = tape if tape_buf is None else tape_buf  # capacity behind Tape / Strings (reuse)
        self._str_buf = strings if str_buf is None else str_buf
        self.records = 0  # filtered streams: matching records of the block
        self.device = -1  # streams: the GPU that parsed the block
        self._owner = None  # view=True: the Context whose pinned block Tape / Strings alias

    @property
    def Message(self):
        if not isinstance(self._msg, bytes):
            self._msg = self._msg.tobytes()
        return self._msg


_DEFAULT = {}


def _default_ctx(device=0):
    c = _DEFAULT.get(device)
    if c is None:
        c = _DEFAULT[device] = Context(device)
    return c


def parse(b, reuse=None, copy_strings=True, ctx=None, view=False):
    """Parse(b, reuse, WithCopyStrings(copy_strings)) -- simdjson_amd64.go:66."""
    return (ctx or _default_ctx()).parse(b, ndjson=False, copy_strings=copy_strings, reuse=reuse, view=view)


def parse_nd(b, reuse=None, copy_strings=True, ctx=None, view=False):
    """ParseND(b, reuse, ...) -- simdjson_amd64.go:82."""
    return (ctx or _default_ctx()).parse(b, ndjson=True, copy_strings=copy_strings, reuse=reuse, view=view)


def stage1(b, ndjson=False, ctx=None):
    return (ctx or _default_ctx()).stage1(b, ndjson=ndjson)
