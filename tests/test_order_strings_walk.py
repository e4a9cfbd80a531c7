"""CPU: the restated "order by <string> limit k" of tests/order_strings_walk.py (the checker of sjhip_order_path_strings), pinned with
hand-written tables -- prefix chains, NUL bytes, unsigned comparison, a descending order with ties, the rows without an OK key last
in both directions, a limit under a selection -- and the serial restatement of the device's rounds (refine) held against it."""
import random

import column_walk as CW
import order_strings_walk as SW
import rows_walk as RW
from test_group_walk import STATUS_DOC
from test_rows_walk import walk_of

OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)


def rows_doc(values):
    return ('{"rows":[%s]}' % ",".join('{"k":%s}' % v for v in values)).encode()


def ordered(values, descending=False, limit=0):
    w = walk_of(rows_doc(values))
    sel = RW.select_rows(w, (b"rows",))
    return SW.order(w, sel, (b"k",), descending, limit), sel


def test_a_proper_prefix_comes_first():
    o, sel = ordered(['"abc"', '"ab"', '""', '"abcd"', '"a"', '"b"', '"ab"'])
    assert o.order == [2, 4, 1, 6, 0, 3, 5] and o.values == [b"", b"a", b"ab", b"ab", b"abc", b"abcd", b"b"]
    assert o.status == [OK] * 7 and (o.records, o.rows) == (1, 7) and o.selection == sel
    o, _ = ordered(['"abc"', '"ab"', '""', '"abcd"', '"a"', '"b"', '"ab"'], descending=True)
    assert o.order == [5, 3, 0, 1, 6, 4, 2]  # the two "ab" in row order: not the ascending list reversed


def test_nul_is_a_byte_like_any_other():
    o, _ = ordered(['"a\\u0000\\u0000"', '"a\\u0000"', '"a"', '"a\\u0000b"', '"a\\u0001"'])
    assert o.order == [2, 1, 0, 3, 4] and o.values == [b"a", b"a\0", b"a\0\0", b"a\0b", b"a\1"]
    o, _ = ordered(['"a\\u0000\\u0000"', '"a\\u0000"', '"a"'], descending=True)
    assert o.order == [0, 1, 2]


def test_bytes_compare_unsigned():
    o, _ = ordered(['"é"', '"z"', '"\U0001F600"', '"Z"', '"\\u00e9"'])
    assert o.values == [b"Z", b"z", b"\xc3\xa9", b"\xc3\xa9", b"\xf0\x9f\x98\x80"] and o.order == [3, 1, 0, 4, 2]  # 0x7A < 0xC3


def test_escaped_spellings_are_one_key():
    o, _ = ordered(['"B"', '"\\u0041"', '"A"', '"\\u0042"'])
    assert o.order == [1, 2, 0, 3] and o.values == [b"A", b"A", b"B", b"B"]


def test_descending_with_ties_is_stable():
    o, _ = ordered(['"x"', '"y"', '"x"', '"z"', '"y"', '"x"'], descending=True)
    assert o.order == [3, 1, 4, 0, 2, 5] and o.values == [b"z", b"y", b"y", b"x", b"x", b"x"]


def test_rows_without_a_string_are_last_in_both_directions():
    w = walk_of(STATUS_DOC)
    sel = RW.select_rows(w, (b"rows",))
    # "k": b, -, (no object), a, null, 12, b, 2^64 - 1, [1], "", a, 12.9, b
    o = SW.order(w, sel, (b"k",))
    assert o.order == [9, 3, 10, 0, 6, 12, 1, 2, 4, 5, 7, 8, 11]
    assert o.status == [OK] * 6 + [NOT_FOUND, NOT_OBJECT, NULL, TYPE, TYPE, TYPE, TYPE]
    assert o.values[:6] == [b"", b"a", b"a", b"b", b"b", b"b"] and o.values[6:] == [None] * 7
    o = SW.order(w, sel, (b"k",), descending=True)
    assert o.order == [0, 6, 12, 3, 10, 9, 1, 2, 4, 5, 7, 8, 11]


def test_limit_narrows_in_document_order():
    o, sel = ordered(['"m"', '"c"', '"m"', '"a"', '"m"'], limit=3)
    assert o.order == [2, 1, 0] and o.values == [b"a", b"c", b"m"] and o.selection[1] == [sel[1][0], sel[1][1], sel[1][3]]
    o, _ = ordered(['"m"', '"c"', '"m"', '"a"', '"m"'], descending=True, limit=2)
    assert o.order == [0, 1] and o.selection[1] == [sel[1][0], sel[1][2]]
    doc = b'{"t":["b","a"]}\n{"t":[]}\n{"t":["c",1,"a"]}'
    w = walk_of(doc, nd=True)
    sel = RW.select_rows(w, (b"t",))
    o = SW.order(w, sel, (), limit=3)  # the rows' own values: a, a, b
    assert o.selection[0] == [0, 2, 2, 3] and o.order == [1, 2, 0] and o.records == 3
    o = SW.order(w, None, (b"t",))  # without a selection the records are the rows; arrays are no strings
    assert o.status == [TYPE] * 3 and o.order == [0, 1, 2]


def test_chunk():
    assert SW.chunk(b"", 0) == 0 and SW.chunk(b"a", 0) == 0x61 << 56 | 1 and SW.chunk(b"a\0", 0) == 0x61 << 56 | 2
    assert SW.chunk(b"abcdefgh", 0) == 0x6162636465666707 and SW.chunk(b"abcdefgh", 7) == 0x68 << 56 | 1
    assert SW.chunk(b"abcdefg", 7) == 0 and SW.chunk(b"abcdefg", 14) == 0
    assert SW.chunk(b"\xff" * 7, 0, True) == 0xF8 and SW.chunk(b"", 0, True) == SW.U64
    assert SW.max_rounds(0) == 1 and SW.max_rounds(6) == 1 and SW.max_rounds(7) == 2 and SW.max_rounds(200) == 29


def test_the_rounds_give_the_rank():
    rnd = random.Random(23)
    alphabet = [0, 1, 0x61, 0x62, 0x7F, 0x80, 0xFF]
    for n, longest in ((1, 3), (2, 0), (50, 3), (300, 9), (300, 16), (400, 30)):
        keys = [bytes(rnd.choice(alphabet[:1 + rnd.randrange(len(alphabet))]) for _ in range(rnd.randrange(longest + 1))) for _ in range(n)]
        for desc in (False, True):
            perm, rounds = SW.refine(keys, desc)
            assert perm == SW.rank(keys, [OK] * n, desc) and rounds <= SW.max_rounds(longest)
    same = [b"abcdefg"] * 5 + [b"abcdefgabcdefg"] * 3  # equal keys of exactly 7 and 14 bytes: the round behind the full chunk ends them
    assert SW.refine(same) == ([0, 1, 2, 3, 4, 5, 6, 7], 3) and SW.refine(same, True) == ([5, 6, 7, 0, 1, 2, 3, 4], 3)
    late = [b"x" * 199 + bytes([c]) for c in (9, 3, 7)]
    assert SW.refine(late) == ([1, 2, 0], 29)
    assert CW.COL_OK == OK and SW.COL_STRING == 4 and SW.CHUNK == 7
