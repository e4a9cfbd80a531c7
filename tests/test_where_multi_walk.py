"""CPU: the restated row predicate over several tests of tests/where_multi_walk.py (the checker of sjhip_where_paths) on
hand-written rows, held against the single-predicate checker tests/where_walk.py: one predicate, NEG, the conjunction of two calls,
De Morgan, and first-member-wins; and its postfix evaluator and validity check on programs written out by hand."""
import itertools

import query_walk as Q
import rows_walk as RW
import where_multi_walk as MW
import where_walk as WW
from test_rows_walk import walk_of

AND, OR, NEG = MW.WHERE_AND, MW.WHERE_OR, MW.WHERE_NEG
DOC = b"\n".join([
    b'{"a":1,"b":"x"}',
    b'{"a":5,"b":null}',
    b'{"a":null}',
    b'{"b":"xy","a":9}',
    b'[1]',                    # the row is no object
    b'{"a":{"v":2},"b":3}',
    b'{"a":"5","c":{"a":5}}',  # a string where a number is asked for
    b'{"x":0}',
])
A_GE_5 = ((b"a",), WW.OP_GE_INT, 5)
B_PREFIX_X = ((b"b",), WW.OP_PREFIX_STRING, b"x")
B_NULL = ((b"b",), Q.OP_IS_NULL, None)


def test_one_predicate_and_its_negation_are_the_single_call():
    w = walk_of(DOC, nd=True)
    for pred in (A_GE_5, B_PREFIX_X, B_NULL, ((b"a",), Q.OP_EXISTS, None), ((b"a", b"v"), WW.OP_LT_FLOAT, 2.5)):
        path, op, want = pred
        assert MW.where_multi(w, None, [pred], bytes([0])) == WW.where(w, None, path, op, want)
        assert MW.where_multi(w, None, [pred], bytes([0, NEG])) == WW.where(w, None, path, op, want, negate=True)
        assert MW.where_multi(w, None, [pred], bytes([0, NEG, NEG])) == WW.where(w, None, path, op, want)
    kept = MW.where_multi(w, None, [A_GE_5], bytes([0]))
    roots = w.records()
    assert kept[1] == [roots[1] + 1, roots[3] + 1] and kept[0] == [0, 0, 1, 1, 2, 2, 2, 2, 2]


def test_and_is_two_successive_calls():
    w = walk_of(DOC, nd=True)
    for x, y in itertools.permutations([A_GE_5, B_PREFIX_X, B_NULL, ((b"a",), Q.OP_EXISTS, None)], 2):
        two = WW.where(w, WW.where(w, None, *x), *y)
        assert MW.where_multi(w, None, [x, y], bytes([0, 1, AND])) == two
        assert MW.where_multi(w, None, [x, y], bytes([1, 0, AND])) == two
    assert MW.where_multi(w, None, [A_GE_5, B_PREFIX_X], bytes([0, 1, AND]))[1] == [w.records()[3] + 1]


def test_de_morgan():
    w = walk_of(DOC, nd=True)
    for x, y in itertools.combinations([A_GE_5, B_PREFIX_X, B_NULL], 2):
        either = MW.where_multi(w, None, [x, y], bytes([0, 1, OR]))
        assert either == MW.where_multi(w, None, [x, y], bytes([0, NEG, 1, NEG, AND, NEG]))
        # ... and against the single calls: the rows either one keeps, in document order
        union = sorted(set(WW.where(w, None, *x)[1]) | set(WW.where(w, None, *y)[1]))
        assert either[1] == union and 0 < len(union) < len(w.records())
    roots = w.records()
    assert MW.where_multi(w, None, [A_GE_5, B_PREFIX_X], bytes([0, 1, OR]))[1] == [roots[r] + 1 for r in (0, 1, 3)]


def test_first_member_wins():
    w = walk_of(b'{"a":1,"a":2}\n{"a":2,"a":1}', nd=True)
    one, two = ((b"a",), Q.OP_EQ_INT, 1), ((b"a",), Q.OP_EQ_INT, 2)
    roots = w.records()
    assert MW.where_multi(w, None, [one], bytes([0]))[1] == [roots[0] + 1]
    assert MW.where_multi(w, None, [two], bytes([0]))[1] == [roots[1] + 1]
    assert MW.where_multi(w, None, [one, two], bytes([0, 1, AND]))[1] == []  # both tests see the FIRST member
    assert MW.where_multi(w, None, [one, two], bytes([0, 1, OR]))[1] == [roots[0] + 1, roots[1] + 1]


def test_on_a_selection_and_on_the_rows_own_value():
    doc = b'{"items":[{"n":1},{"n":5},7,{"n":9}]}\n{"items":null}\n{"items":[]}\n{"items":[{"n":2},{"n":8}]}\n{"x":1}'
    w = walk_of(doc, nd=True)
    sel = RW.select_rows(w, (b"items",))
    lo, hi = ((b"n",), WW.OP_GE_INT, 2), ((b"n",), WW.OP_LT_INT, 9)
    rng = MW.where_multi(w, sel, [lo, hi], bytes([0, 1, AND]))  # a range on one path
    assert rng == WW.where(w, WW.where(w, sel, *lo), *hi)
    assert rng[0] == [0, 1, 1, 1, 3, 3] and rng[2] == sel[2] and rng[1] == [sel[1][1], sel[1][4], sel[1][5]]
    num = ((), WW.OP_GT_FLOAT, 0.0)  # the empty path next to a path: the scalar row or a row with a large n
    got = MW.where_multi(w, sel, [num, hi], bytes([0, 1, NEG, OR]))
    assert got[1] == [sel[1][2], sel[1][3]]
    assert MW.where_multi(w, rng, [lo], bytes([0, NEG])) == ([0] * 6, [], sel[2])  # no rows kept, and on from there
    assert MW.where_multi(w, ([0] * 6, [], sel[2]), [lo], bytes([0])) == ([0] * 6, [], sel[2])


def test_evaluator_and_validity_by_hand():
    assert MW.evaluate(bytes([0, 1, AND, 2, OR]), [1, 0, 1]) is True
    assert MW.evaluate(bytes([0, 1, 2, OR, AND]), [0, 1, 1]) is False
    assert MW.evaluate(bytes([0, 1, NEG, AND]), [1, 0]) is True
    ok = (MW.PROG_OK, 0)
    assert MW.check_program(bytes([0]), 1) == ok and MW.check_program(bytes([0, 0, AND, 1, OR]), 2) == ok
    assert MW.check_program(b"", 1) == (MW.PROG_LENGTH, 0) and MW.check_program(bytes([0] + [NEG] * 64), 1) == (MW.PROG_LENGTH, 0)
    assert MW.check_program(bytes([0] + [NEG] * 63), 1) == ok
    assert MW.check_program(bytes([AND]), 1) == (MW.PROG_UNDERFLOW, 0) and MW.check_program(bytes([NEG, 0]), 1) == (MW.PROG_UNDERFLOW, 0)
    assert MW.check_program(bytes([0, 1, AND, OR]), 2) == (MW.PROG_UNDERFLOW, 3)
    assert MW.check_program(bytes([0, 1]), 2) == (MW.PROG_LEFT, 2)
    assert MW.check_program(bytes([0, 0, OR]), 2) == (MW.PROG_UNUSED, 1)
    assert MW.check_program(bytes([0, 2, OR]), 2) == (MW.PROG_PREDICATE, 1)
    assert MW.check_program(bytes([0, 0x83]), 1) == (MW.PROG_BYTE, 1) and MW.check_program(bytes([0, 16, OR]), 16) == (MW.PROG_BYTE, 1)
