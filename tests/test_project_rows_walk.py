"""CPU: the serial restatement of sjhip_marshal_rows_paths (tests/project_rows_walk.py), pinned from outside itself on twitter.json
statuses, parking-citations lines and a hand-made document with nested, scalar and array rows: every line, parsed by the oracle and
marshaled again, is that line; for rows without duplicate keys json.loads of the line is the dict built by navigating json.loads of
the source row along the paths; absent columns are left out, or None under nulls."""
import json

import pytest

import fixtures
import oracle_lib as O
import project_rows_walk as PW
import rows_walk as RW
from test_filter_rows_walk import walk_of

ABSENT = object()


def navigate(row, path):
    """what FindElement gives on a row without duplicate keys: into objects only"""
    for key in path:
        if not isinstance(row, dict) or key.decode() not in row:
            return ABSENT
        row = row[key.decode()]
    return row


def expected(row, columns, names, nulls):
    out = {}
    for path, name in zip(columns, names):
        x = navigate(row, path)
        if x is ABSENT and not nulls:
            continue
        out[name.decode()] = None if x is ABSENT else x
    return out


def remarshaled(line):
    ref = O.parse(line, ndjson=False)
    assert ref.rc == 0, line[:80]
    rc, out = O.marshal_json(ref.tape, ref.strings, line)
    assert rc == 0
    return out


def check(w, rows, sources, columns, names=None):
    """sources: json.loads of every row's source text (ABSENT: the row has duplicate keys and is not compared) -> the lines
    without nulls"""
    for nulls in (True, False):
        text, offsets = PW.project_rows(w, rows, columns, names, nulls)
        lines = text.split(b"\n")
        assert len(lines) == len(rows) and offsets[-1] == len(text) + 1
        assert [text[offsets[i]:offsets[i + 1] - 1] for i in range(len(rows))] == lines
        for line, src in zip(lines, sources):
            assert remarshaled(line) == line
            if src is not ABSENT:
                assert json.loads(line) == expected(src, columns, PW.column_names(columns, names), nulls), line[:120]
    return lines


def test_twitter_statuses():
    doc = fixtures.load("twitter")
    w = walk_of(doc, nd=False)
    rows = RW.select_rows(w, (b"statuses",))[1]
    statuses = json.loads(doc)["statuses"]
    assert len(rows) == len(statuses) > 50
    columns = [(b"id",), (b"user", b"screen_name"), (b"retweet_count",), (b"user",), (b"entities", b"hashtags"), (b"text",),
               (b"retweeted_status", b"user", b"name"), (b"user", b"name", b"nothing")]
    names = [b"id", b"screen_name", b"retweets", b"user", b"tags", b"text", b"rt", b"none"]
    lines = check(w, rows, statuses, columns, names)
    assert any(b'"rt":' in l for l in lines) and not all(b'"rt":' in l for l in lines) and not any(b'"none"' in l for l in lines)
    check(w, rows, statuses, columns[:3])  # named by the last keys


def test_parking_citations_lines():
    doc = fixtures.load("parking-citations")
    w = walk_of(doc)
    roots = [r + 1 for r in w.records()][:300]
    sources = [json.loads(l) for l in doc.split(b"\n")[:300]]
    some = sorted(sources[0])[:3]
    assert len(some) == 3
    check(w, roots, sources, [(k.encode(),) for k in some] + [(b"no such field",)])


HAND = ['{"a":{"b":{"c":[1,{"d":"e"}],"n":null},"s":"x\\ny"},"k":1.5,"u":{"name":"N","id":7}}',
        '{"a":5,"k":{"deep":[{}]},"u":{"name":{"first":"F"}}}',
        '"a scalar row"', "12", "-0.5", "true", "null",
        '[{"a":{"b":1}},2]', "[]", "{}",
        '{"u":{"id":[]},"a":{"b":"only b"}}']
HAND_DUP = ['{"a":1,"a":{"b":2},"k":"first","k":"second"}', '{"u":{"name":"one","name":"two"},"u":{"name":"three"}}']
HAND_COLUMNS = [(b"a", b"b"), (b"a",), (), (b"k",), (b"u", b"name"), (b"u",), (b"a", b"b", b"n"), (b"a", b"b", b"c")]
HAND_NAMES = [b"a.b", b"a", b"row", b"k", b"who", b"u", b"n", b"c"]


def hand_walk(texts):
    doc = ("[" + ",".join(texts) + "]").encode()
    w = walk_of(doc, nd=False)
    rows = RW.select_rows(w, ())[1]
    assert len(rows) == len(texts)
    return w, rows


def test_hand_made_rows():
    w, rows = hand_walk(HAND)
    sources = [json.loads(t) for t in HAND]
    lines = check(w, rows, sources, HAND_COLUMNS, HAND_NAMES)
    assert lines[0] == b'{"a.b":{"c":[1,{"d":"e"}],"n":null},"a":{"b":{"c":[1,{"d":"e"}],"n":null},"s":"x\\ny"},"row":' + \
        HAND[0].encode() + b',"k":1.5,"who":"N","u":{"name":"N","id":7},"n":null,"c":[1,{"d":"e"}]}'
    assert lines[2] == b'{"row":"a scalar row"}' and lines[6] == b'{"row":null}' and lines[7] == b'{"row":[{"a":{"b":1}},2]}'
    # NOT_OBJECT on the way (a.b where a is a number) is absent like NOT_FOUND; a present null is null either way
    no, yes = (PW.project_rows(w, rows[:2], [(b"a", b"b"), (b"a", b"b", b"n")], None, nulls)[0].split(b"\n") for nulls in (False, True))
    assert no == [b'{"b":{"c":[1,{"d":"e"}],"n":null},"n":null}', b"{}"]
    assert yes == [no[0], b'{"b":null,"n":null}']


def test_duplicate_keys_the_first_one_wins():
    w, rows = hand_walk(HAND_DUP)
    lines = check(w, rows, [ABSENT] * len(rows), [(b"a", b"b"), (b"k",), (b"u", b"name"), (b"a",)])
    assert lines == [b'{"k":"first","a":1}', b'{"name":"one"}']


@pytest.mark.parametrize("name, want", [(b"", b'""'), (b'q"b\\s', b'"q\\"b\\\\s"'), (bytes(range(0x20)), None), ("é中  \U0001f600".encode(), None)])
def test_names_are_escaped_as_escape_bytes_does(name, want):
    got = PW.name_text(name)
    if want is None:  # control bytes are \b \f \n \r \t or \u00xx; everything from 0x20 up stands for itself (U+2028/2029 too)
        want = b'"' + b"".join({8: b"\\b", 12: b"\\f", 10: b"\\n", 13: b"\\r", 9: b"\\t"}.get(c, b"\\u%04x" % c) if c < 0x20 else bytes([c])
                                for c in name) + b'"'
    assert got == want
    w, rows = hand_walk(['{"x":1}'])
    assert PW.project_rows(w, rows, [(b"x",), (b"x",)], [name, name])[0] == b"{" + want + b":1," + want + b":1}"
