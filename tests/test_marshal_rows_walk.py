"""CPU: the serial restatement of sjhip_marshal_rows (tests/marshal_rows_walk.py) against the oracle.  The expected text is never
the restatement's own: for container rows it is the corresponding line of the oracle's MarshalJSON of the ND document made of the
rows' texts, on an ND parse whose records are all containers the rows joined are the oracle's whole MarshalJSON byte for byte, and
scalar rows are compared with their known compact texts."""
import pytest

import marshal_rows_walk as MW
import oracle_lib as O
import rows_walk as RW
from test_filter_rows_walk import SCALAR_ROWS, items_doc, kinds_rows, walk_of


def oracle_lines(texts):
    """the lines of the oracle's MarshalJSON of the ND document whose lines are `texts` (container texts only)"""
    doc = "\n".join(texts).encode()
    ref = O.parse(doc, ndjson=True)
    assert ref.rc == 0
    rc, out = O.marshal_json(ref.tape, ref.strings, doc)
    assert rc == 0
    return out.split(b"\n")


@pytest.mark.parametrize("keep", ["all", "every third", "odd"])
def test_container_rows_equal_the_oracles_lines(keep):
    doc, order, box = items_doc(kinds_rows(61))
    w = walk_of(doc)
    rows = RW.select_rows(w, (b"items",))[1]
    assert len(rows) == 61 and all(box)
    kept = [r for r in range(61) if {"all": True, "every third": r % 3 == 0, "odd": r % 2 == 1}[keep]]
    text, offsets = MW.marshal_rows(w, [rows[r] for r in kept])
    want = oracle_lines([order[r] for r in kept])
    assert text.split(b"\n") == want
    assert len(offsets) == len(kept) + 1 and offsets[-1] == len(text) + 1
    assert [text[offsets[i]:offsets[i + 1] - 1] for i in range(len(kept))] == want


def test_all_records_joined_equal_the_whole_marshal_json():
    texts = kinds_rows(40)
    doc = "\n".join(texts).encode()
    w = walk_of(doc)
    roots = [r + 1 for r in w.records()]
    rc, want = O.marshal_json(w.t, [x for x in w.s], doc)
    assert rc == 0
    assert MW.marshal_rows(w, roots)[0] == want


def test_scalar_rows_are_their_own_text():
    doc, order, box = items_doc(kinds_rows(30), scalars_every=4)
    w = walk_of(doc)
    rows = RW.select_rows(w, (b"items",))[1]
    assert 0 < box.count(False) < len(box)
    lines = MW.marshal_rows(w, rows)[0].split(b"\n")
    assert len(lines) == len(rows)
    assert [l for l, b in zip(lines, box) if b] == oracle_lines([t for t, b in zip(order, box) if b])
    assert [l.decode() for l, b in zip(lines, box) if not b] == [t for t, b in zip(order, box) if not b]  # (SCALAR_ROWS are compact)
    # the scalars the issue names
    doc = b'["a\\"b",-3,1e21,null,1e20,-0.0,18446744073709551615,true,false,""]'
    w = walk_of(doc, nd=False)
    rows = RW.select_rows(w, ())[1]
    assert [MW.row_text(w, v).decode() for v in rows] == ['"a\\"b"', "-3", "1e+21", "null", "100000000000000000000", "-0", "18446744073709551615",
                                                           "true", "false", '""']
    assert set(SCALAR_ROWS) >= {'""', "null"}


def test_no_rows_and_offsets():
    doc, order, box = items_doc(kinds_rows(5))
    w = walk_of(doc)
    assert MW.marshal_rows(w, []) == (b"", [0])
    rows = RW.select_rows(w, (b"items",))[1]
    text, offsets = MW.marshal_rows(w, rows[:1])
    assert offsets == [0, len(text) + 1] and b"\n" not in text
