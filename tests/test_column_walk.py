"""CPU: the restated conversions of tests/column_walk.py (the checker of the device columns) against the reference's own examples
(ExampleIter_FindElement parsed_json_test.go:1235-1283, ExampleParsedJson_ForEach :1285-1315, ExampleObject_FindPath
parsed_object_test.go:247-307, ExampleArray :309-378), the conversion edges of Iter.Int / Uint / Float on hand-made tapes, and
query_walk.element_is -- the checker of sjhip_count_where_path -- on random documents."""
import random

import column_walk as CW
import oracle_lib as O
import query_walk as Q
from test_query_walk import FINDPATH_INPUT  # the document of the reference's FindPath / FindElement / Array examples

TAG = 56
STRINGBUFBIT = Q.STRINGBUFBIT


def walk_of(doc, nd=False, copy=True):
    ref = O.parse(doc, ndjson=nd, copy_strings=copy)
    assert ref.rc == 0
    return Q.Walk(ref.tape, ref.strings, doc[ref.msg_off:ref.msg_off + ref.msg_len])


def at(w, path):
    (root,) = w.records()
    return w.find_path(root, list(path))


def test_example_iter_find_element():  # Image/Thumbnail/Width: Type int, StringCvt "100"
    for copy in (True, False):
        w = walk_of(FINDPATH_INPUT, copy=copy)
        v = at(w, [b"Image", b"Thumbnail", b"Width"])
        assert CW.text(w, v, True) == (CW.COL_OK, b"100")
        assert CW.text(w, v, False) == (CW.COL_TYPE, b"")
        assert CW.convert(w, v, CW.COL_INT) == (CW.COL_OK, 100)
        assert CW.convert(w, v, CW.COL_FLOAT) == (CW.COL_OK, CW.f2bits(100.0))
        offs, data, sts = CW.string_column(w, [b"Image", b"Thumbnail", b"Width"], True)
        assert (offs, data, sts) == ([0, 3], b"100", [CW.COL_OK])


def test_example_parsed_json_for_each():  # Image/URL: StringCvt "http://example.com/example.gif"
    w = walk_of(b'{"Image":{"URL":"http://example.com/example.gif"}}')
    assert CW.text(w, at(w, [b"Image", b"URL"]), True) == (CW.COL_OK, b"http://example.com/example.gif")
    assert CW.string_column(w, [b"Image", b"URL"], False)[1] == b"http://example.com/example.gif"


def test_example_object_find_path():  # Image/Thumbnail/Url: String "http://www.example.com/image/481989943"
    for copy in (True, False):
        w = walk_of(FINDPATH_INPUT, copy=copy)
        v = at(w, [b"Image", b"Thumbnail", b"Url"])
        assert CW.text(w, v, False) == (CW.COL_OK, b"http://www.example.com/image/481989943")
        assert CW.convert(w, v, CW.COL_INT) == (CW.COL_TYPE, 0)


def test_example_array():  # Image/IDs is an array: StringCvt of it is an error; its elements are ints
    w = walk_of(FINDPATH_INPUT)
    v = at(w, [b"Image", b"IDs"])
    assert CW.text(w, v, True) == (CW.COL_TYPE, b"")
    assert CW.string_column(w, [b"Image", b"IDs"], True) == ([0, 0], b"", [CW.COL_TYPE])
    assert CW.column(w, [b"Image", b"IDs", b"0"], CW.COL_INT) == ([0], [CW.COL_NOT_OBJECT])
    assert CW.column(w, [b"Image", b"Nope"], CW.COL_INT) == ([0], [CW.COL_NOT_FOUND])
    assert CW.column(w, [b"Alt", b"x"], CW.COL_INT) == ([0], [CW.COL_NOT_OBJECT])
    assert CW.column(w, [b"Image", b"Animated"], CW.COL_BOOL) == ([0], [CW.COL_OK])
    assert CW.text(w, at(w, [b"Image", b"Animated"]), True) == (CW.COL_OK, b"false")


# ---- hand-made tapes: {"k": <value>} with the value's tag and raw word as given ---------------------------------------------
def one_value(tag, raw=None):
    two = raw is not None
    n = 8 if two else 7
    t = [(ord("r") << TAG) | n,
         (ord("{") << TAG) | (n - 1),
         (ord('"') << TAG) | STRINGBUFBIT | 0, 1,
         (ord(tag) << TAG)]
    if two:
        t.append(raw)
    t += [(ord("}") << TAG) | 1, (ord("r") << TAG) | 0]
    assert len(t) == n
    return Q.Walk(t, b"k", b"")


def conv(tag, raw, kind):
    w = one_value(tag, raw)
    return CW.convert(w, at(w, [b"k"]), kind)


def test_conversion_edges():
    F, I, U, B = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT, CW.COL_BOOL
    OK, RANGE, TYPE, NULL = CW.COL_OK, CW.COL_RANGE, CW.COL_TYPE, CW.COL_NULL
    fb = CW.f2bits
    assert conv("d", fb(2.0 ** 63), I) == (OK, 1 << 63)            # MinInt64: the amd64 conversion of 2^63
    assert conv("d", fb(-(2.0 ** 63)), I) == (OK, 1 << 63)
    assert conv("d", fb(2.0 ** 63 * (1 + 2.0 ** -52)), I) == (RANGE, 0)
    assert conv("d", fb(-(2.0 ** 63) * (1 + 2.0 ** -52)), I) == (RANGE, 0)
    assert conv("d", fb(2.0 ** 64), U) == (OK, 0)                  # 0: the amd64 conversion of 2^64
    assert conv("d", fb(2.0 ** 64 * (1 + 2.0 ** -52)), U) == (RANGE, 0)
    assert conv("d", fb(2.0 ** 63), U) == (OK, 1 << 63)
    assert conv("d", fb(-1.5), U) == (RANGE, 0)
    assert conv("d", fb(-0.0), U) == (OK, 0)                       # -0 < 0 is false
    assert conv("d", fb(-0.0), F) == (OK, 1 << 63)                 # keeps its sign
    assert conv("d", fb(-2.75), I) == (OK, (-2) & CW.U64)          # truncation
    assert conv("l", (-5) & CW.U64, U) == (RANGE, 0)
    assert conv("l", (-5) & CW.U64, I) == (OK, (-5) & CW.U64)
    assert conv("l", (-5) & CW.U64, F) == (OK, fb(-5.0))
    assert conv("u", (1 << 63), I) == (RANGE, 0)
    assert conv("u", (1 << 63) - 1, I) == (OK, (1 << 63) - 1)
    assert conv("u", CW.U64, F) == (OK, fb(2.0 ** 64))              # float64(MaxUint64) rounds up
    assert conv("l", (1 << 53) + 1, F) == (OK, fb(2.0 ** 53))      # ... and to even
    for kind in (F, I, U, B):
        assert conv("n", None, kind) == (NULL, 0)
    assert conv("t", None, B) == (OK, 1) and conv("f", None, B) == (OK, 0)
    assert conv("t", None, I) == (TYPE, 0) and conv("l", 1, B) == (TYPE, 0)
    w = one_value("n")
    assert CW.text(w, at(w, [b"k"]), False) == (NULL, b"") and CW.text(w, at(w, [b"k"]), True) == (OK, b"null")
    w = one_value("d", fb(-0.0))
    assert CW.text(w, at(w, [b"k"]), True) == (OK, b"-0")
    w = one_value("d", fb(1e21))
    assert CW.text(w, at(w, [b"k"]), True) == (OK, b"1e+21")
    w = one_value("d", fb(1e-7))
    assert CW.text(w, at(w, [b"k"]), True) == (OK, b"1e-7")
    w = one_value("l", (-(1 << 63)) & CW.U64)
    assert CW.text(w, at(w, [b"k"]), True) == (OK, b"-9223372036854775808")
    w = one_value("u", CW.U64)
    assert CW.text(w, at(w, [b"k"]), True) == (OK, b"18446744073709551615")


# ---- against element_is on random documents -----------------------------------------------------------------------------------
EDGE_NUMS = ["9223372036854775808.0", "-9223372036854775808.0", "18446744073709551616.0", "-0.0", "0", "-0", "1e308", "4.9e-324",
             "2.2250738585072014e-308", "0.1000000000000000055511151231257827", "9223372036854775807", "9223372036854775808",
             "18446744073709551615", "-9223372036854775808", "-1", "1.5", "-2.5", "1e21", "123456789012345678901234567890", "3"]


def random_value(rnd, depth=0):
    r = rnd.random()
    if r < 0.35:
        return rnd.choice(EDGE_NUMS)
    if r < 0.45:
        return str(rnd.randint(-2 ** 64, 2 ** 64))
    if r < 0.55:
        return rnd.choice(["true", "false", "null"])
    if r < 0.7:
        return rnd.choice(['"x"', '""', '"a\\"b\\u00e9"', '"3"'])
    if depth < 2 and r < 0.85:
        return "{" + ",".join('"%s":%s' % (rnd.choice("abk"), random_value(rnd, depth + 1)) for _ in range(rnd.randint(0, 3))) + "}"
    return "[" + ",".join(random_value(rnd, depth + 1) for _ in range(rnd.randint(0, 2))) + "]" if depth < 2 else "1"


def test_agrees_with_element_is_on_random_documents():
    rnd = random.Random(5)
    lines = []
    for _ in range(400):
        lines.append("[" + random_value(rnd) + "]" if rnd.random() < 0.1 else  # (the reference accepts no scalar roots)
                     "{" + ",".join('"%s":%s' % (rnd.choice("abk"), random_value(rnd)) for _ in range(rnd.randint(0, 4))) + "}")
    doc = "\n".join(lines).encode()
    ops = {CW.COL_INT: Q.OP_EQ_INT, CW.COL_UINT: Q.OP_EQ_UINT, CW.COL_FLOAT: Q.OP_EQ_FLOAT, CW.COL_BOOL: Q.OP_EQ_BOOL}
    for copy in (True, False):
        w = walk_of(doc, nd=True, copy=copy)
        seen = 0
        for path in ([b"a"], [b"k"], [b"a", b"b"], [b"k", b"a", b"b"]):
            for root in w.records():
                v = w.find_path(root, path)
                if v >= Q.NOT_OBJECT:
                    continue
                for kind, op in ops.items():
                    st, x = CW.convert(w, v, kind)
                    assert (st == CW.COL_NULL) == w.element_is(v, Q.OP_IS_NULL)
                    if kind == CW.COL_FLOAT:
                        wants = [CW.bits2f(x), 0.0, 1.5, 2.0 ** 64, 1e308]
                        for want in wants:
                            assert w.element_is(v, op, want) == (st == CW.COL_OK and CW.bits2f(x) == want), (path, want)
                    elif kind == CW.COL_BOOL:
                        for want in (0, 1):
                            assert w.element_is(v, op, bool(want)) == (st == CW.COL_OK and x == want)
                    else:
                        signed = lambda b: b - (1 << 64) if kind == CW.COL_INT and b >= 1 << 63 else b
                        for want in (signed(x), 0, 3, (1 << 63) if kind == CW.COL_UINT else -(1 << 63), signed(x) + 1):
                            assert w.element_is(v, op, want) == (st == CW.COL_OK and signed(x) == want), (path, kind, want)
                    seen += st == CW.COL_OK
                stb, b = CW.text(w, v, False)
                assert w.element_is(v, Q.OP_EQ_STRING, b) == (stb == CW.COL_OK)
        assert seen > 200
