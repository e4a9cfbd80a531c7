"""The reference's array conversions at a path, restated on (Tape, Strings.B, Message) arrays -- the checker of the device list
columns sjhip_extract_path_list / sjhip_extract_path_list_strings (test infrastructure, like column_walk.py).

  array_at       FindElement(path...) (query_walk.Walk.find_path) then Iter.Array (parsed_json.go:1022-1025)
  as_float       Array.AsFloat      parsed_array.go:145-181
  as_integer     Array.AsInteger    parsed_array.go:185-232
  as_uint64      Array.AsUint64     parsed_array.go:236-283
  as_string      Array.AsString     parsed_array.go:287-314
  as_string_cvt  Array.AsStringCvt  parsed_array.go:319-344
  list_column          -> (list_offsets [records + 1], value bits [elems], statuses [records])
  list_string_column   -> (list_offsets [records + 1], str_offsets [elems + 1], data, statuses [records])

A status names the error the reference's call chain would have returned (COL_*, include/sjhip.h); the reference returns at the
first element it cannot convert, so a record's status is that of its first failing element and a record that is not OK owns no
elements.  `null` at the path is COL_NULL (the scalar columns' convention); a null ELEMENT is a type error like any other tag.
Numbers are returned as their 64-bit patterns.  Float text comes from the oracle's appendFloat (oracle_lib.format_float), as in
column_walk.text.  Pinned by tests/test_list_walk.py."""
import column_walk as CW
from column_walk import COL_FLOAT, COL_INT, COL_NOT_FOUND, COL_NOT_OBJECT, COL_NULL, COL_OK, COL_RANGE, COL_TYPE, COL_UINT, U64  # noqa: F401
from query_walk import MASK, NOT_OBJECT

TWO_63 = 2.0 ** 63  # math.MaxInt64 and -math.MinInt64 as float64 constants


def array_at(w, root, path):
    """-> (index of the array's '[' word, COL_OK) or (None, status)"""
    v = w.find_path(root, list(path))
    if v == NOT_OBJECT:
        return None, COL_NOT_OBJECT
    if v > NOT_OBJECT:
        return None, COL_NOT_FOUND
    tag = chr(w.t[v] >> 56)
    if tag == "n":
        return None, COL_NULL  # (the convention of the scalar columns; the reference: "next item is not array")
    if tag != "[":
        return None, COL_TYPE  # parsed_json.go:1023-1024 "next item is not array"
    return v, COL_OK


def _numbers(w, v, one):
    """the readArray loop shared by AsFloat / AsInteger / AsUint64: a.off walks the words behind the '['"""
    out, off = [], v + 1
    while True:
        tag = chr(w.t[off] >> 56)
        off += 1
        if tag == "]":  # TagArrayEnd: parsed_array.go:173 / 224 / 275
            return COL_OK, out
        if tag not in "dlu":  # default: parsed_array.go:175-176 / 226-227 / 277-278 "unable to convert type ..."
            return COL_TYPE, []
        st, x = one(tag, w.t[off])
        if st != COL_OK:
            return st, []
        out.append(x)
        off += 1


def as_float(w, v):
    def one(tag, raw):
        if tag == "d":
            return COL_OK, raw  # parsed_array.go:162 math.Float64frombits
        if tag == "l":
            return COL_OK, CW.f2bits(float(raw - (1 << 64) if raw >= 1 << 63 else raw))  # :167 float64(int64(...))
        return COL_OK, CW.f2bits(float(raw))  # :172 float64(uint64)
    return _numbers(w, v, one)


def as_integer(w, v):
    def one(tag, raw):
        if tag == "d":
            d = CW.bits2f(raw)
            if d > TWO_63:  # parsed_array.go:202-204 "float value overflows int64"
                return COL_RANGE, 0
            if d < -TWO_63:  # :205-207 "float value underflows int64"
                return COL_RANGE, 0
            return COL_OK, (1 << 63) if d >= TWO_63 else int(d) & U64  # :208 int64(val); 2^63: the amd64 "integer indefinite"
        if tag == "l":
            return COL_OK, raw  # :213
        if raw > (1 << 63) - 1:  # :220-222 "unsigned integer value overflows int64"
            return COL_RANGE, 0
        return COL_OK, raw  # :223
    return _numbers(w, v, one)


def as_uint64(w, v):
    def one(tag, raw):
        if tag == "d":
            d = CW.bits2f(raw)
            if d > TWO_63:  # parsed_array.go:253-255 `val > math.MaxInt64` (not MaxUint64, unlike Iter.Uint)
                return COL_RANGE, 0
            if d < 0:  # :256-258 "float value is negative" (-0.0 < 0 is false)
                return COL_RANGE, 0
            return COL_OK, int(d)  # :259 uint64(val); exactly 2^63 is 1 << 63
        if tag == "l":
            if raw >= 1 << 63:  # :265-267 "int64 value is negative"
                return COL_RANGE, 0
            return COL_OK, raw  # :268
        return COL_OK, raw  # :274
    return _numbers(w, v, one)


def _texts(w, v, cvt):
    """AsString / AsStringCvt: Array.Iter + AdvanceIter over the elements (a container element is one element)"""
    out = []
    i, end = v + 1, (w.t[v] & MASK) - 1
    while i < end:
        tag = chr(w.t[i] >> 56)
        if not cvt and tag != '"':  # parsed_array.go:310-311 "element in array is not string, but ..."
            return COL_TYPE, []
        st, b = CW.text(w, i, cvt)  # :305 elem.String() / :337 elem.StringCvt()
        if st != COL_OK:
            return st, []  # (StringCvt of an object or array: "cannot convert type ... to string")
        out.append(b)
        i = w.skip(i)
    return COL_OK, out  # TypeNone: :302-303 / :334-335


def as_string(w, v):
    return _texts(w, v, False)


def as_string_cvt(w, v):
    return _texts(w, v, True)


NUMERIC = {COL_FLOAT: as_float, COL_INT: as_integer, COL_UINT: as_uint64}


def list_column(w, path, kind):
    """-> (list_offsets, value bits, statuses)"""
    offs, vals, sts = [0], [], []
    for root in w.records():
        v, st = array_at(w, root, path)
        if v is not None:
            st, xs = NUMERIC[kind](w, v)
            vals += xs
        offs.append(len(vals))
        sts.append(st)
    return offs, vals, sts


def list_string_column(w, path, cvt):
    """-> (list_offsets, str_offsets, data, statuses)"""
    offs, soffs, parts, sts, at = [0], [0], [], [], 0
    for root in w.records():
        v, st = array_at(w, root, path)
        if v is not None:
            st, bs = _texts(w, v, cvt)
            for b in bs:
                parts.append(b)
                at += len(b)
                soffs.append(at)
        offs.append(len(soffs) - 1)
        sts.append(st)
    return offs, soffs, b"".join(parts), sts
