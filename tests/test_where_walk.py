"""CPU: the restated row predicate of tests/where_walk.py (the checker of sjhip_where_path), pinned two ways: a table written out by
hand on one small document -- every operator and its NOT, against a missing path, a non-object on the way and at the root, null,
a string where a number is asked for, 1.5 under *_INT, -1 under *_UINT, floats of exactly 2^63 and 2^64, -0.0 and an escaped
string under PREFIX_STRING --, and Python's own comparisons on json.loads values over the number texts of tests/number_cases.py
that are finite and inside the range of the operator's kind."""
import json
import random

import column_walk as CW
import number_cases as NC
import query_walk as Q
import where_walk as WW
from test_rows_walk import walk_of

OK = 0
NAN = float("nan")
PATH = (b"a", b"v")
HAND_DOC = b"\n".join([
    b'{"x":1}',                              # 0  the path is missing
    b'{"a":5}',                              # 1  a non-object on the way
    b'[1]',                                  # 2  ... and at the root
    b'{"a":{"v":null}}',                     # 3
    b'{"a":{"v":"12"}}',                     # 4  a string where a number is asked for
    b'{"a":{"v":1.5}}',                      # 5  Int and Uint truncate: 1
    b'{"a":{"v":-1}}',                       # 6  a range error under *_UINT
    b'{"a":{"v":9223372036854775808.0}}',    # 7  2^63: MinInt64 under *_INT (the amd64 result), 2^63 under *_UINT
    b'{"a":{"v":18446744073709551616.0}}',   # 8  2^64: a range error under *_INT, 0 under *_UINT (the amd64 result)
    b'{"a":{"v":-0.0}}',                     # 9  0 under *_INT and *_UINT, equal to 0.0 and not below it
    b'{"a":{"v":"a\\"b\\u0041c"}}',          # 10 a"bAc once unescaped
    b'{"a":{"v":7}}',                        # 11
    b'{"a":{"v":18446744073709551615}}',     # 12 MaxUint64: a range error under *_INT, 2^64 as a float
    b'{"a":{"v":true}}',                     # 13
])
N = 14
W = WW
HAND = [  # (op, want, the records kept)
    (Q.OP_EXISTS, None, list(range(3, 14))), (Q.OP_EQ_STRING, b"12", [4]), (Q.OP_EQ_INT, 1, [5]), (Q.OP_EQ_UINT, 0, [8, 9]),
    (Q.OP_EQ_FLOAT, 0.0, [9]), (Q.OP_EQ_BOOL, True, [13]), (Q.OP_IS_NULL, None, [3]),
    (W.OP_LT_INT, 1, [6, 7, 9]), (W.OP_LE_INT, 1, [5, 6, 7, 9]), (W.OP_GT_INT, 0, [5, 11]), (W.OP_GE_INT, 0, [5, 9, 11]),
    (W.OP_GE_INT, -(1 << 63), [5, 6, 7, 9, 11]), (W.OP_LE_INT, -(1 << 63), [7]), (W.OP_GT_INT, (1 << 63) - 1, []),
    (W.OP_LT_UINT, 1, [8, 9]), (W.OP_LE_UINT, 1, [5, 8, 9]), (W.OP_GT_UINT, 7, [7, 12]), (W.OP_GE_UINT, 7, [7, 11, 12]),
    (W.OP_GE_UINT, 1 << 63, [7, 12]), (W.OP_GT_UINT, 1 << 63, [12]), (W.OP_LT_UINT, 0, []),
    (W.OP_LT_FLOAT, 0.0, [6]), (W.OP_LE_FLOAT, 0.0, [6, 9]), (W.OP_LE_FLOAT, -0.0, [6, 9]), (W.OP_GT_FLOAT, 2.0 ** 63, [8, 12]),
    (W.OP_GE_FLOAT, 2.0 ** 63, [7, 8, 12]), (W.OP_GT_FLOAT, -0.0, [5, 7, 8, 11, 12]), (W.OP_GE_FLOAT, NAN, []), (W.OP_LT_FLOAT, NAN, []),
    (W.OP_PREFIX_STRING, b'a"bA', [10]), (W.OP_PREFIX_STRING, b"", [4, 10]), (W.OP_PREFIX_STRING, b"12", [4]),
    (W.OP_PREFIX_STRING, b"123", []), (W.OP_PREFIX_STRING, b'a"bAc', [10]), (W.OP_PREFIX_STRING, b"a\\", []),
]


def test_hand_written_table():
    w = walk_of(HAND_DOC, nd=True)
    roots = w.records()
    assert len(roots) == N and {op for op, _, _ in HAND} == set(WW.ALL_OPS)
    for op, want, kept in HAND:
        for negate in (False, True):
            expect = [r for r in range(N) if (r in kept) != negate]
            offs, index, sts = WW.where(w, None, PATH, op, want, negate)
            assert index == [roots[r] + 1 for r in expect], (op, want, negate)
            assert sts == [OK] * N and offs == [sum(e < r for e in expect) for r in range(N + 1)], (op, want, negate)


def test_narrowing_a_selection():
    doc = b'{"items":[{"n":1},{"n":5},7,{"n":9}]}\n{"items":null}\n{"items":[]}\n{"items":[{"n":2},{"n":8}]}\n{"x":1}'
    w = walk_of(doc, nd=True)
    import rows_walk as RW
    sel = RW.select_rows(w, (b"items",))
    assert sel[0] == [0, 4, 4, 4, 6, 6] and sel[2] == [OK, CW.COL_NULL, OK, OK, CW.COL_NOT_FOUND]
    first = WW.where(w, sel, (b"n",), WW.OP_GE_INT, 5)
    assert first[0] == [0, 2, 2, 2, 3, 3] and first[1] == [sel[1][1], sel[1][3], sel[1][5]] and first[2] == sel[2]
    both = WW.where(w, first, (b"n",), WW.OP_LT_INT, 9)  # successive calls: the conjunction
    assert both[0] == [0, 1, 1, 1, 2, 2] and both[1] == [sel[1][1], sel[1][5]]
    others = WW.where(w, sel, (b"n",), WW.OP_GE_INT, 5, negate=True)  # the row that is no object is among them
    assert others[0] == [0, 2, 2, 2, 3, 3] and others[1] == [sel[1][0], sel[1][2], sel[1][4]]
    none = WW.where(w, both, (b"n",), Q.OP_IS_NULL)
    assert none == ([0] * 6, [], sel[2]) and WW.where(w, none, (b"n",), Q.OP_EXISTS) == none
    # an empty path: the row's own value
    w = walk_of(b'[3,"a",null,7.5,-2]')
    sel = RW.select_rows(w, ())
    assert WW.where(w, sel, (), WW.OP_GT_FLOAT, 0.0) == ([0, 2], [sel[1][0], sel[1][3]], [OK])
    assert WW.where(w, sel, (), WW.OP_GT_FLOAT, 0.0, negate=True)[1] == [sel[1][1], sel[1][2], sel[1][4]]


WANTS = {CW.COL_INT: [0, -1, 1000, (1 << 63) - 1, -(1 << 63)], CW.COL_UINT: [0, 1, 1 << 63, (1 << 64) - 1],
         CW.COL_FLOAT: [0.0, -1.5, 1e300, 5e-324, 2.0 ** 63]}
PY = {"<": lambda a, b: a < b, "<=": lambda a, b: a <= b, ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}


def test_python_comparisons_on_the_number_texts():
    texts = NC.sample(random.Random(20261017), 2500) + ["0", "-0.0", "1.5", "-1", "9223372036854775807", "-9223372036854775808",
                                                        "18446744073709551615", "9223372036854775808"]
    w = walk_of("\n".join('{"v":%s}' % t for t in texts).encode(), nd=True)
    roots = w.records()
    assert len(roots) == len(texts)
    checked = {k: 0 for k in WANTS}
    for t, root in zip(texts, roots):
        x = json.loads(t)
        v = w.find_path(root, [b"v"])
        for op in WW.ORDER_OPS:
            kind, rel = WW.KIND_OF[op], WW.RELATION[(op - WW.OP_LT_INT) % 4]
            if kind == CW.COL_INT:
                inside, got = -(1 << 63) <= x < (1 << 63), int(x)
            elif kind == CW.COL_UINT:
                inside, got = 0 <= x < (1 << 64), int(x)
            else:
                try:
                    inside, got = True, float(x)
                except OverflowError:
                    continue
            if not inside:
                continue
            checked[kind] += 1
            for want in WANTS[kind]:
                assert WW.satisfies(w, v, op, want) == PY[rel](got, want), (t, op, want)
    assert min(checked.values()) > 2000, checked
    kept = WW.where(w, None, (b"v",), WW.OP_GE_FLOAT, 1.0)[1]
    assert kept == [r + 1 for t, r in zip(texts, roots) if float(json.loads(t)) >= 1.0]
