"""The reference's value conversions at a path, restated on (Tape, Strings.B, Message) arrays -- the checker of the device
columns sjhip_extract_path / sjhip_extract_path_strings (test infrastructure, like oracle/ and query_walk.py).

  convert        Iter.Float / Int / Uint (parsed_json.go:560-749) and Iter.Bool (:867-875) of the element at a tape index
  text           Iter.StringBytes (:751-760) or Iter.StringCvt (:775-800)
  column         FindElement(path...) (:833-865, query_walk.Walk.find_path) + convert on the root of every record
  string_column  FindElement(path...) + text on every record, in Arrow's large-string layout (offsets, data, status)

A status names the reference's error the host API would have returned (COL_*, include/sjhip.h); a value that is not OK is 0
and a text that is not OK is empty.  Numbers are returned as their 64-bit patterns (the bits of a double, the two's
complement of an int64), so that the device's values compare as bits.  Float text comes from the oracle's appendFloat
(oracle_lib.format_float).  Pinned by tests/test_column_walk.py."""
import struct

import oracle_lib as O
from query_walk import NOT_OBJECT, Walk  # noqa: F401  (Walk: what callers build the checker on)

COL_FLOAT, COL_INT, COL_UINT, COL_BOOL = range(4)
COL_OK, COL_NOT_FOUND, COL_NOT_OBJECT, COL_TYPE, COL_NULL, COL_RANGE = range(6)

U64 = (1 << 64) - 1


def f2bits(d):
    return struct.unpack("<Q", struct.pack("<d", d))[0]


def bits2f(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def convert(w, v, kind):
    """(status, value bits) of Iter.Float / Int / Uint / Bool for the element whose tag word is w.t[v]"""
    tag = chr(w.t[v] >> 56)
    if tag == "n":
        return COL_NULL, 0  # "unable to convert type null ..." / "value is not bool"
    if kind == COL_BOOL:
        return (COL_OK, 1 if tag == "t" else 0) if tag in "tf" else (COL_TYPE, 0)
    if tag not in "lud":
        return COL_TYPE, 0
    raw = w.t[v + 1]
    as_i = raw - (1 << 64) if raw >= 1 << 63 else raw
    if kind == COL_FLOAT:
        if tag == "d":
            return COL_OK, raw
        return COL_OK, f2bits(float(as_i if tag == "l" else raw))
    if kind == COL_INT:
        if tag == "l":
            return COL_OK, raw
        if tag == "u":
            return (COL_RANGE, 0) if raw > (1 << 63) - 1 else (COL_OK, raw)
        d = bits2f(raw)
        # `v > math.MaxInt64` / `v < math.MinInt64` compare with the float64 constants 2^63 / -2^63; int64(v) of exactly 2^63 is
        # the amd64 conversion's "integer indefinite", MinInt64
        if d > 2.0 ** 63 or d < -(2.0 ** 63):
            return COL_RANGE, 0
        return COL_OK, (1 << 63) if d >= 2.0 ** 63 else int(d) & U64
    if kind == COL_UINT:
        if tag == "u":
            return COL_OK, raw
        if tag == "l":
            return (COL_RANGE, 0) if as_i < 0 else (COL_OK, raw)
        d = bits2f(raw)
        # `v > math.MaxUint64` compares with the float64 2^64, so exactly 2^64 passes, and uint64(v) of it is 0 on amd64
        if d < 0.0 or d > 2.0 ** 64:
            return COL_RANGE, 0
        return COL_OK, 0 if d >= 2.0 ** 64 else int(d)
    raise ValueError(kind)


def text(w, v, cvt):
    """(status, bytes) of Iter.StringBytes (cvt False) / Iter.StringCvt (cvt True) for the element at w.t[v]"""
    tag = chr(w.t[v] >> 56)
    if tag == '"':
        return COL_OK, w.string_at(v)
    if not cvt:
        return (COL_NULL if tag == "n" else COL_TYPE), b""  # "value is not string"
    if tag in "lud":
        raw = w.t[v + 1]
        if tag == "l":
            return COL_OK, str(raw - (1 << 64) if raw >= 1 << 63 else raw).encode()  # strconv.FormatInt
        if tag == "u":
            return COL_OK, str(raw).encode()  # strconv.FormatUint
        return COL_OK, O.format_float(raw).encode()  # floatToString -> appendFloat
    lit = {"t": b"true", "f": b"false", "n": b"null"}.get(tag)
    if lit is None:
        return COL_TYPE, b""  # "cannot convert type object / array to string"
    return COL_OK, lit


def _at_path(w, root, path):
    v = w.find_path(root, list(path))
    if v == NOT_OBJECT:
        return None, COL_NOT_OBJECT
    if v > NOT_OBJECT:
        return None, COL_NOT_FOUND
    return v, COL_OK


def column(w, path, kind):
    """-> (value bits, statuses), one entry per record"""
    vals, sts = [], []
    for root in w.records():
        v, st = _at_path(w, root, path)
        x = 0
        if v is not None:
            st, x = convert(w, v, kind)
        vals.append(x)
        sts.append(st)
    return vals, sts


def string_column(w, path, cvt):
    """-> (offsets [records + 1], data, statuses)"""
    offs, parts, sts, at = [0], [], [], 0
    for root in w.records():
        v, st = _at_path(w, root, path)
        b = b""
        if v is not None:
            st, b = text(w, v, cvt)
        parts.append(b)
        at += len(b)
        offs.append(at)
        sts.append(st)
    return offs, b"".join(parts), sts
