"""CPU: the serial restatement of sjhip_filter_rows (tests/filter_rows_walk.py) against the oracle.  The documents are built from
known row texts, so the expected answer is the oracle's ParseND of those texts joined by newlines -- not the restatement's own:
NDJSON records {"pre":..,"items":[rows],"post":[..]} with 0 / 1 / 3 / 7 rows each and rows of every kind; scalar rows skipped and
counted; no rows; and a hand-written table of tiny tapes."""
import numpy as np
import pytest

import filter_rows_walk as FW
import oracle_lib as O
import query_walk as Q
import rows_walk as RW

BIG = 18446744073709551615
RAW_BRACKET = 6557241057451442176  # an integer whose value word has the top byte '['
# container rows of every kind the issue names: nested objects and arrays, {} and [], escaped and \u strings, empty strings, floats
# and large uint64, rows without strings
ROW_KINDS = [
    '{"a":1,"b":"x"}',
    '{"o":{"p":{"q":[1,2,{"r":"deep"}]}},"t":[[],[[]],{}]}',
    "{}",
    "[]",
    '{"e":"a\\"b\\\\c\\/d\\n\\t","u":"\\u00e9\\u4e2d\\ud83d\\ude00"}',
    '{"":"","k":""}',
    '[1.5,-0.0,1e308,4.9e-324,%d,9223372036854775808,-9223372036854775808]' % BIG,
    "[[1,2],[3,[4,[5]]],true,false,null]",
    '["only","strings","","in","an","array"]',
    '{"n":%d,"s":"after a raw word that looks like a tag"}' % RAW_BRACKET,
    '[{"a":"HOND"},{"a":["x",{"b":"y"}]},"tail"]',
    '{"long":"%s"}' % ("0123456789abcdef" * 9),
]
SCALAR_ROWS = ['"a string row"', "42", "-1.25", "true", "false", "null", '""']


def items_doc(rows, counts=(0, 1, 3, 7), scalars_every=0):
    """NDJSON whose records hold the rows, counts[k % len] of them in record k -- and, every scalars_every-th row, a scalar in front
    of it.  -> (document, [row texts in document order], [is the row a container])"""
    lines, order, box, at, k, s = [], [], [], 0, 0, 0
    while at < len(rows):
        take = counts[k % len(counts)]
        mine = []
        for text in rows[at:at + take]:
            if scalars_every and (len(order) % scalars_every) == 0:
                mine.append(SCALAR_ROWS[s % len(SCALAR_ROWS)])
                order.append(mine[-1])
                box.append(False)
                s += 1
            mine.append(text)
            order.append(text)
            box.append(True)
        lines.append('{"pre":{"k":%d,"s":"before %d"},"items":[%s],"post":["after",%d,{"z":"%s"}]}' % (k, k, ",".join(mine), k, "z" * (k % 5)))
        at += take
        k += 1
    return "\n".join(lines).encode(), order, box


def kinds_rows(n):
    """n rows cycling through ROW_KINDS, each made distinct by a numbered member or element"""
    out = []
    for r in range(n):
        text = ROW_KINDS[r % len(ROW_KINDS)]
        if r >= len(ROW_KINDS):
            text = '{"r":%d,"v":%s,"w":"row %d"}' % (r, text, r) if r % 2 else "[%d,%s]" % (r, text)
        out.append(text)
    return out


def walk_of(doc, nd=True):
    ref = O.parse(doc, ndjson=nd)
    assert ref.rc == 0
    return Q.Walk(ref.tape, ref.strings, doc)


def oracle_of(texts):
    """(Tape, Strings.B) ParseND returns for the document whose lines are `texts`; two empty arrays for none"""
    if not texts:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint8)
    ref = O.parse("\n".join(texts).encode(), ndjson=True)
    assert ref.rc == 0
    return ref.tape, ref.strings


def same(got, want, what=None):
    tape, strings = got[0], got[1]
    assert np.array_equal(np.array(tape, dtype=np.uint64), want[0]), what
    assert np.array_equal(np.frombuffer(bytes(strings), dtype=np.uint8), want[1]), what


@pytest.mark.parametrize("keep", ["all", "drop every third", "every third", "odd"])
def test_rows_of_every_kind_equal_the_oracle(keep):
    doc, order, box = items_doc(kinds_rows(61))
    w = walk_of(doc)
    rows = RW.select_rows(w, (b"items",))[1]
    assert len(rows) == len(order) == 61 and all(box)
    pick = {"all": lambda r: True, "drop every third": lambda r: r % 3 != 2, "every third": lambda r: r % 3 == 0,
            "odd": lambda r: r % 2 == 1}[keep]
    kept = [r for r in range(61) if pick(r)]
    tape, strings, skipped = FW.filter_rows(w, [rows[r] for r in kept])
    want = oracle_of([order[r] for r in kept])
    assert skipped == 0 and len(tape) > 4 * len(kept) and len(strings) > len(kept)
    same((tape, strings), want, keep)


def test_scalar_rows_are_skipped_and_counted():
    doc, order, box = items_doc(kinds_rows(30), scalars_every=4)
    w = walk_of(doc)
    rows = RW.select_rows(w, (b"items",))[1]
    assert len(rows) == len(order) and 0 < box.count(False) < len(box)
    tape, strings, skipped = FW.filter_rows(w, rows)
    assert skipped == box.count(False)
    same((tape, strings), oracle_of([t for t, b in zip(order, box) if b]))
    # scalars only
    scalars = [i for i, b in zip(rows, box) if not b]
    assert FW.filter_rows(w, scalars) == ([], b"", len(scalars))


def test_no_rows():
    doc, order, box = items_doc(kinds_rows(5))
    assert FW.filter_rows(walk_of(doc), []) == ([], b"", 0)


def test_records_as_rows():
    """the selection sjhip_where_path makes without sjhip_select_rows: the root values of the records"""
    texts = kinds_rows(40)
    doc = "\n".join(texts).encode()
    w = walk_of(doc)
    roots = [r + 1 for r in w.records()]
    same(FW.filter_rows(w, roots), oracle_of(texts))
    same(FW.filter_rows(w, roots[5::7]), oracle_of(texts[5::7]))


def test_result_larger_than_the_source():
    doc = b"[" + b",".join([b"[]"] * 50) + b"]"
    w = walk_of(doc, nd=False)
    rows = RW.select_rows(w, ())[1]
    tape, strings, skipped = FW.filter_rows(w, rows)
    assert len(tape) == 200 > len(w.t) == 104 and strings == b"" and skipped == 0
    same((tape, strings), oracle_of(["[]"] * 50))


# ---- a hand-written table of tiny tapes ---------------------------------------------------------------------------------------------
def T(tag, payload=0):
    return (ord(tag) << 56) | payload


SB = Q.STRINGBUFBIT
TINY = [
    # (document, its tape, its Strings.B, the rows, the result's tape, the result's Strings.B, skipped)
    (b'[{"a":"x"},7,[]]',
     [T("r", 14), T("[", 13), T("{", 8), T('"', SB + 0), 1, T('"', SB + 1), 1, T("}", 2), T("l"), 7, T("[", 12), T("]", 10), T("]", 1), T("r", 0)],
     b"ax", [2, 8, 10],
     [T("r", 8), T("{", 7), T('"', SB + 0), 1, T('"', SB + 1), 1, T("}", 1), T("r", 0), T("r", 12), T("[", 11), T("]", 9), T("r", 8)],
     b"ax", 1),
    # a raw word that looks like '[' is copied as it is
    (b'[[%d,"s"]]' % RAW_BRACKET,
     [T("r", 10), T("[", 9), T("[", 8), T("l"), RAW_BRACKET, T('"', SB + 0), 1, T("]", 2), T("]", 1), T("r", 0)],
     b"s", [2],
     [T("r", 8), T("[", 7), T("l"), RAW_BRACKET, T('"', SB + 0), 1, T("]", 1), T("r", 0)],
     b"s", 0),
    # a dropped row that owns strings leaves a gap in Strings.B: the kept row's offsets move down
    (b'[{"k":"dropped"},{"q":"kept"}]',
     [T("r", 16), T("[", 15), T("{", 8), T('"', SB + 0), 1, T('"', SB + 1), 7, T("}", 2),
      T("{", 14), T('"', SB + 8), 1, T('"', SB + 9), 4, T("}", 8), T("]", 1), T("r", 0)],
     b"kdroppedqkept", [8],
     [T("r", 8), T("{", 7), T('"', SB + 0), 1, T('"', SB + 1), 4, T("}", 1), T("r", 0)],
     b"qkept", 0),
    # a row whose only strings are empty owns no bytes, and the row behind it starts where it would have
    (b'[{"":""},["z"]]',
     [T("r", 14), T("[", 13), T("{", 8), T('"', SB + 0), 0, T('"', SB + 0), 0, T("}", 2), T("[", 12), T('"', SB + 0), 1, T("]", 8), T("]", 1), T("r", 0)],
     b"z", [2, 8],
     [T("r", 8), T("{", 7), T('"', SB + 0), 0, T('"', SB + 0), 0, T("}", 1), T("r", 0), T("r", 14), T("[", 13), T('"', SB + 0), 1, T("]", 9), T("r", 8)],
     b"z", 0),
]


@pytest.mark.parametrize("case", range(len(TINY)))
def test_tiny_tapes(case):
    doc, src, src_strings, rows, want, want_strings, skipped = TINY[case]
    ref = O.parse(doc)
    assert ref.rc == 0 and ref.tape.tolist() == src and ref.strings.tobytes() == src_strings  # the table's source is the oracle's
    assert FW.filter_rows(Q.Walk(src, src_strings, doc), rows) == (want, want_strings, skipped)
