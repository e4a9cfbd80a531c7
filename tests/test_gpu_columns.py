"""GPU: columns at a path (sjhip_extract_path / sjhip_extract_path_strings + sjhip_fetch_path_strings) against the restated
conversions of tests/column_walk.py over the oracle's parse -- values as bits, statuses and string columns byte for byte --
and against the existing path queries on the same paths (count_where_path, find_path); a sharded result against the same
message parsed whole; the lifecycle of the string column."""
import random
import struct

import numpy as np
import pytest

import column_walk as CW
import fixtures
import oracle_lib as O
import query_walk as Q
from test_gpu_parse import ctx  # noqa: F401
from test_query_walk import FINDPATH_INPUT

pytestmark = pytest.mark.gpu

KINDS = (CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT, CW.COL_BOOL)


def oracle_walk(doc, nd, copy):
    ref = O.parse(doc, ndjson=nd, copy_strings=copy)
    assert ref.rc == 0
    return Q.Walk(ref.tape, ref.strings, doc[ref.msg_off:ref.msg_off + ref.msg_len])


def check_numbers(ctx, w, path):
    for kind in KINDS:
        vals, st = ctx.extract_path(path, kind)
        want_v, want_s = CW.column(w, path, kind)
        assert np.array_equal(st, np.array(want_s, dtype=np.uint8)), (path, kind)
        if kind == CW.COL_BOOL:
            assert vals.dtype == np.uint8 and np.array_equal(vals, np.array(want_v, dtype=np.uint8)), (path, kind)
        else:
            assert vals.dtype == ctx._COL_DTYPES[kind]
            assert np.array_equal(vals.view(np.uint64), np.array(want_v, dtype=np.uint64)), (path, kind)


def check_strings(ctx, w, path):
    for cvt in (False, True):
        off, data, st = ctx.extract_path_strings(path, cvt=cvt)
        want_o, want_d, want_s = CW.string_column(w, path, cvt)
        assert np.array_equal(st, np.array(want_s, dtype=np.uint8)), (path, cvt)
        assert off.dtype == np.uint64 and np.array_equal(off, np.array(want_o, dtype=np.uint64)), (path, cvt)
        assert data == want_d, (path, cvt)


def check_doc(ctx, doc, nd, paths, copy):
    w = oracle_walk(doc, nd, copy)
    ctx.parse(doc, ndjson=nd, copy_strings=copy)
    for path in paths:
        check_numbers(ctx, w, path)
        check_strings(ctx, w, path)
    return w


# ---- seeded random records --------------------------------------------------------------------------------------------------
EDGES = ["9223372036854775808.0", "-9223372036854775808.0", "9223372036854777856.0", "18446744073709551616.0",
         "18446744073709555712.0", "-0.0", "-0", "0", "1e308", "-1e308", "4.9e-324", "2.2250738585072014e-308", "1e-7", "1e21",
         "123456.789e-3", "0.1000000000000000055511151231257827", "3.141592653589793238462643383279", "9223372036854775807",
         "9223372036854775808", "18446744073709551615", "-9223372036854775808", "-9223372036854775809", "-1", "1", "100"]
STRINGS = ['""', '"x"', '"HOND"', '"a\\"b\\\\c\\/d\\n\\t"', '"\\u00e9\\u4e2d\\ud83d\\ude00"', '"3"', '"true"', '"caf\u00e9 \u00e9"']
STRINGS += ['"' + "a long string, " * 3 + '\\u00e9"', '"' + "x" * 3000 + '\\n"']  # (longer than a lane copies alone)
KEYS = ['"a"', '"b"', '"c"', '""', '"\\u0061"', '"a\\"q"']  # (the fifth is "a" through an escape)


def rvalue(rnd, depth):
    r = rnd.random()
    if r < 0.3:
        return rnd.choice(EDGES)
    if r < 0.4:
        return str(rnd.randint(-2 ** 63, 2 ** 64 - 1)) if rnd.random() < 0.7 else repr(rnd.uniform(-1e6, 1e6))
    if r < 0.5:
        return rnd.choice(["true", "false", "null"])
    if r < 0.65:
        return rnd.choice(STRINGS)
    if depth < 3 and r < 0.9:
        return robj(rnd, depth + 1)
    if depth < 3:
        return "[" + ",".join(rvalue(rnd, depth + 1) for _ in range(rnd.randint(0, 3))) + "]"
    return "7"


def robj(rnd, depth):
    return "{" + ",".join("%s:%s" % (rnd.choice(KEYS), rvalue(rnd, depth)) for _ in range(rnd.randint(0, 5))) + "}"


def random_nd(seed, n):
    rnd = random.Random(seed)
    lines = []
    for _ in range(n):
        r = rnd.random()
        lines.append(robj(rnd, 0) if r < 0.9 else "[" + rvalue(rnd, 1) + "]")  # (the reference accepts no scalar roots)
    return "\n".join(lines).encode()


RANDOM_PATHS = [(b"a",), (b"b",), (b"",), (b'a"q',), (b"a", b"b"), (b"b", b"a"), (b"a", b""), (b"a", b"b", b"c"), (b"c", b"c", b"a")]


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_random_records(ctx, copy):
    doc = random_nd(11, 3000)
    w = check_doc(ctx, doc, True, RANDOM_PATHS, copy)
    # every status and kind occurs
    seen = set()
    for path in RANDOM_PATHS:
        for kind in KINDS:
            seen |= set(CW.column(w, path, kind)[1])
    assert seen == set(range(6)), seen


def test_fixtures(ctx):
    park = fixtures.load("parking-citations") * 7
    for copy in (True, False):
        w = check_doc(ctx, park, True, [(b"Make",), (b"Fine",), (b"Latitude",)], copy)
        for path in ((b"Make",), (b"Fine",), (b"Latitude",)):
            _, st = ctx.extract_path(path, CW.COL_FLOAT)
            assert np.all(st == CW.COL_TYPE), path  # every value of the parking records is a string
    check_doc(ctx, fixtures.load("twitter"), False, [(b"search_metadata", b"count"), (b"search_metadata", b"max_id_str")], True)
    vals, st = ctx.extract_path((b"search_metadata", b"count"), CW.COL_INT)
    assert st.tolist() == [CW.COL_OK] and vals.tolist() == [100]
    check_doc(ctx, fixtures.load("canada"), False, [(b"type",)], False)
    off, data, st = ctx.extract_path_strings((b"type",))
    assert data == b"FeatureCollection" and off.tolist() == [0, 17]
    for copy in (True, False):
        check_doc(ctx, FINDPATH_INPUT, False, [(b"Image", b"Thumbnail", b"Width"), (b"Image", b"Thumbnail", b"Url"), (b"Image", b"IDs"),
                                               (b"Alt",), (b"Image", b"Animated"), (b"Image", b"IDs", b"0")], copy)
        off, data, st = ctx.extract_path_strings((b"Image", b"Thumbnail", b"Width"), cvt=True)
        assert data == b"100" and st.tolist() == [CW.COL_OK]  # ExampleIter_FindElement


def test_consistent_with_the_path_queries(ctx):
    doc = random_nd(12, 2000)
    for copy in (True, False):
        ctx.parse(doc, ndjson=True, copy_strings=copy)
        for path in RANDOM_PATHS:
            idx = ctx.find_path(*path)
            ops = {CW.COL_INT: ctx.OP_EQ_INT, CW.COL_UINT: ctx.OP_EQ_UINT, CW.COL_FLOAT: ctx.OP_EQ_FLOAT, CW.COL_BOOL: ctx.OP_EQ_BOOL}
            for kind, op in ops.items():
                vals, st = ctx.extract_path(path, kind)
                assert np.array_equal(st == CW.COL_NOT_FOUND, idx == Q.NOT_FOUND), (path, kind)
                assert np.array_equal(st == CW.COL_NOT_OBJECT, idx == Q.NOT_OBJECT), (path, kind)
                exists = (st != CW.COL_NOT_FOUND) & (st != CW.COL_NOT_OBJECT)
                assert int(exists.sum()) == ctx.count_where_path(path, ctx.OP_EXISTS)
                assert int((st == CW.COL_NULL).sum()) == ctx.count_where_path(path, ctx.OP_IS_NULL)
                ok = vals[st == CW.COL_OK]
                for v in list(dict.fromkeys(ok.tolist()))[:6]:
                    if kind == CW.COL_FLOAT:
                        n = int((ok == v).sum())  # (a comparison of doubles, like EQ_FLOAT: -0.0 == 0.0)
                    else:
                        n = int((ok == ok.dtype.type(v)).sum())
                    want = bool(v) if kind == CW.COL_BOOL else v
                    assert n == ctx.count_where_path(path, op, want), (path, kind, v)
            off, data, st = ctx.extract_path_strings(path)
            ok_idx = np.nonzero(st == CW.COL_OK)[0]
            for r in ok_idx[:5]:
                s = data[int(off[r]):int(off[r + 1])]
                if len(s) > 1024:
                    continue  # (longer than a query value may be)
                want = sum(1 for rr in ok_idx if data[int(off[rr]):int(off[rr + 1])] == s)
                assert ctx.count_where_path(path, ctx.OP_EQ_STRING, s) == want, (path, s)


def test_sharded_result_equals_whole():
    import sjhip
    park = fixtures.load("parking-citations")
    doc = park * 4 + random_nd(13, 9000) + b"\n" + park * 3
    assert len(doc) > (2 << 20)
    paths = [(b"Make",), (b"Latitude",), (b"a",), (b"a", b"b")]
    one = sjhip.Context(0)
    for copy in (True, False):
        one.parse(doc, ndjson=True, copy_strings=copy)
        want = {}
        for path in paths:
            want[path] = ([one.extract_path(path, k) for k in KINDS], [one.extract_path_strings(path, cvt=c) for c in (False, True)])
        with fixtures.nd_shard_limits(2 << 20, 1 << 20):
            many = sjhip.Context(0)
            many.parse(doc, ndjson=True, copy_strings=copy)
        w = oracle_walk(doc, True, copy)
        for path in paths:
            nums, strs = want[path]
            for k, (v1, s1) in zip(KINDS, nums):
                v2, s2 = many.extract_path(path, k)
                assert np.array_equal(s1, s2) and np.array_equal(v1, v2), (path, k, copy)
            for cvt, (o1, d1, s1) in zip((False, True), strs):
                o2, d2, s2 = many.extract_path_strings(path, cvt=cvt)
                assert np.array_equal(o1, o2) and d1 == d2 and np.array_equal(s1, s2), (path, cvt, copy)
            check_strings(many, w, path)
        many.close()
    one.close()


def test_lifecycle(ctx):
    import sjhip
    L = sjhip.lib()
    doc = b'{"s":"abc","n":1}\n{"s":"de","n":2.5}\n{"n":null}'
    ctx.parse(doc, ndjson=True)
    # too small a cap_records: SJHIP_ERR_ARG with the record count set
    blob, lens, n = ctx._keys([b"n"])
    import ctypes as C
    cnt = C.c_size_t(0)
    vals, st = np.zeros(2, np.float64), np.zeros(2, np.uint8)
    assert L.sjhip_extract_path(ctx._h, blob, lens, n, CW.COL_FLOAT, vals.ctypes.data, st.ctypes.data, 2, C.byref(cnt)) == 5
    assert cnt.value == 3
    assert L.sjhip_extract_path(ctx._h, blob, lens, n, 9, vals.ctypes.data, st.ctypes.data, 2, C.byref(cnt)) == 5
    # fetch with no column built
    fresh = sjhip.Context(0)
    fresh.parse(doc, ndjson=True)
    with pytest.raises(sjhip.ParseError) as e:
        fresh.fetch_path_strings(3, 5)
    assert e.value.code == 5 and "no string column" in str(e.value)
    fresh.close()
    # extract, parse another document: the column is gone; extract again: no stale bytes
    nr, nb = ctx.extract_path_strings((b"s",), fetch=False)
    assert (nr, nb) == (3, 5)
    ctx.parse(b'{"s":"z"}\n{"s":""}', ndjson=True)
    with pytest.raises(sjhip.ParseError):
        ctx.fetch_path_strings(nr, nb)
    off, data, st = ctx.extract_path_strings((b"s",))
    assert off.tolist() == [0, 1, 1] and data == b"z" and st.tolist() == [0, 0]
    # MarshalJSON / filter_where / serialize / the other queries between extract and fetch leave the column alone
    big = fixtures.load("parking-citations")
    ctx.parse(big, ndjson=True, key_flags=True)
    w = oracle_walk(big, True, True)
    want = CW.string_column(w, (b"Make",), True)
    nr, nb = ctx.extract_path_strings((b"Make",), cvt=True, fetch=False)
    ctx.marshal_json()
    ctx.filter_where(b"Make", b"HOND")
    ctx.serialize()
    ctx.find_path(b"Color")
    ctx.extract_path((b"Fine",), CW.COL_INT)
    off, data, st = ctx.fetch_path_strings(nr, nb)
    assert off.tolist() == want[0] and data == want[1] and st.tolist() == want[2]
    # a column of empty strings: offsets all 0
    ctx.parse(b'{"e":""}\n{"e":""}\n{"e":""}', ndjson=True)
    off, data, st = ctx.extract_path_strings((b"e",))
    assert off.tolist() == [0, 0, 0, 0] and data == b"" and st.tolist() == [0, 0, 0]
    # a column with no OK record at all
    off, data, st = ctx.extract_path_strings((b"nope",))
    assert off.tolist() == [0, 0, 0, 0] and data == b"" and st.tolist() == [CW.COL_NOT_FOUND] * 3
    # a bool column and a number at 2^63 / 2^64
    ctx.parse(b'{"b":true,"x":9223372036854775808.0,"y":18446744073709551616.0}', ndjson=True)
    assert ctx.extract_path((b"b",), CW.COL_BOOL)[0].tolist() == [1]
    assert ctx.extract_path((b"x",), CW.COL_INT)[0].tolist() == [-(2 ** 63)]
    v, s = ctx.extract_path((b"y",), CW.COL_UINT)
    assert v.tolist() == [0] and s.tolist() == [CW.COL_OK]
    assert struct.pack("<d", ctx.extract_path((b"x",), CW.COL_FLOAT)[0][0]) == struct.pack("<d", 2.0 ** 63)
