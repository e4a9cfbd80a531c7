"""CPU: the restated row selection of tests/rows_walk.py (the checker of sjhip_select_rows), pinned two ways: small documents with
the rows written out by hand -- every status, nested elements that must not become rows, duplicate keys, the root array --, and
Python's json as the outside arbiter on the fixtures whose rows lie in an array: twitter (statuses), github_events (the root
array), citm_catalog (performances)."""
import json

import column_walk as CW
import fixtures
import oracle_lib as O
import query_walk as Q
import rows_walk as RW
import table_walk as TW

OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)


def walk_of(doc, nd=False, copy=True):
    ref = O.parse(doc, ndjson=nd, copy_strings=copy)
    assert ref.rc == 0, doc
    return Q.Walk(ref.tape, ref.strings, doc[ref.msg_off:ref.msg_off + ref.msg_len])


def tags(w, index):
    return "".join(chr(w.t[i] >> 56) for i in index)


# one NDJSON input whose records hit every status (tests/test_gpu_rows.py runs the device on it)
STATUS_DOC = b"\n".join([
    b'{"x":1}',                                                 # the path is missing
    b'{"a":5}',                                                 # a non-object on the way (a.items)
    b'[1,2]',                                                   # ... and at the root
    b'{"a":{"items":null}}',                                    # the element is null
    b'{"a":{"items":"str"}}', b'{"a":{"items":7}}', b'{"a":{"items":{"k":[1]}}}',  # a string, a number, an object
    b'{"a":{"items":[]}}',                                      # an empty array
    b'{"a":{"items":[1,"two",3.5,true,false,null]}}',           # scalars only
    b'{"a":{"items":[{"k":[{"n":1},{"n":2}]},[[{"m":1}],2],"s",[],{},7]}}',  # nested elements are no rows
    b'{"a":{"items":[1],"items":[2,3]},"a":{"items":[4,5,6]}}',  # duplicate keys: the first wins at every level
    b'{"a":{"x":[9]},"a":{"items":[4]}}',                       # ... also where the first has no such member
])
STATUS_PATH = (b"a", b"items")
STATUS_WANT = ([0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 12, 13, 13],
               [NOT_FOUND, NOT_OBJECT, NOT_OBJECT, NULL, TYPE, TYPE, TYPE, OK, OK, OK, OK, NOT_FOUND], "l\"dtfn" + "{[\"[{l" + "l")


def test_every_status():
    w = walk_of(STATUS_DOC, nd=True)
    offs, index, sts = RW.select_rows(w, STATUS_PATH)
    assert (offs, sts, tags(w, index)) == STATUS_WANT
    assert index == sorted(set(index))
    # the root array of the third record, and only that one, under the empty path
    offs, index, sts = RW.select_rows(w, ())
    assert offs == [0, 0, 0, 2] + [2] * 9 and sts == [TYPE, TYPE, OK] + [TYPE] * 9 and tags(w, index) == "ll"


def test_hand_written_rows():
    doc = b'{"k":3,"items":[{"id":1,"t":["a","b"]},{"id":2.5,"t":[]},"x",{"id":"z","u":{"id":9}}]}'
    w = walk_of(doc)
    offs, index, sts = RW.select_rows(w, (b"items",))
    assert offs == [0, 4] and sts == [OK] and tags(w, index) == '{{"{'
    rw = RW.on_rows(w, (b"items",))
    assert RW.find_path(rw, (b"id",)) == [index[0] + 3, index[1] + 3, Q.NOT_OBJECT, index[3] + 3]
    assert RW.find_path(rw, (b"u", b"id")) == [Q.NOT_FOUND, Q.NOT_FOUND, Q.NOT_OBJECT, index[3] + 10]
    assert RW.column(rw, (b"id",), CW.COL_INT) == ([1, 2, 0, 0], [OK, OK, NOT_OBJECT, TYPE])
    assert RW.string_column(rw, (b"id",), True) == ([0, 1, 4, 4, 5], b"12.5z", [OK, OK, NOT_OBJECT, OK])
    assert RW.list_string_column(rw, (b"t",), False) == ([0, 2, 2, 2, 2], [0, 1, 2], b"ab", [OK, OK, NOT_OBJECT, NOT_FOUND])
    assert RW.count_where_path(rw, (b"id",), Q.OP_EXISTS) == 3 and RW.count_where_path(rw, (b"id",), Q.OP_EQ_INT, 2) == 1
    assert RW.project_keys(rw, (b"t", b"id"))[0] == [(1, index[0] + 3), (0, index[0] + 7)]
    table = RW.table(rw, [((b"id",), CW.COL_FLOAT), ((b"u", b"id"), TW.COL_STRING_CVT)])
    assert table[0][1] == [OK, OK, NOT_OBJECT, TYPE] and table[1] == ([0, 0, 0, 0, 1], b"9", [NOT_FOUND, NOT_FOUND, NOT_OBJECT, OK])
    # NDJSON lines exploded into one row per item
    w = walk_of(b'{"order":1,"items":[{"q":1},{"q":2}]}\n{"order":2,"items":[]}\n{"order":3,"items":[{"q":3}]}', nd=True)
    assert RW.select_rows(w, (b"items",))[::2] == ([0, 2, 2, 3], [OK, OK, OK])
    assert RW.column(RW.on_rows(w, (b"items",)), (b"q",), CW.COL_INT) == ([1, 2, 3], [OK] * 3)


def strings_of(col):
    offs, data, sts = col
    assert all(s == OK for s in sts)
    return [data[offs[k]:offs[k + 1]].decode() for k in range(len(sts))]


def test_fixtures_against_json():
    doc = fixtures.load("twitter")
    w, want = walk_of(doc), json.loads(doc)["statuses"]
    offs, index, sts = RW.select_rows(w, (b"statuses",))
    assert offs == [0, 100] and sts == [OK] and tags(w, index) == "{" * 100 and len(want) == 100
    rw = RW.RowWalk(w, index)
    assert strings_of(RW.string_column(rw, (b"user", b"screen_name"), False)) == [s["user"]["screen_name"] for s in want]
    assert RW.column(rw, (b"id",), CW.COL_INT) == ([s["id"] for s in want], [OK] * 100)
    assert RW.select_rows(w, ())[2] == [TYPE]  # the root of twitter.json is an object

    doc = fixtures.load("github_events")
    w, want = walk_of(doc), json.loads(doc)
    offs, index, sts = RW.select_rows(w, ())
    assert offs == [0, len(want)] and sts == [OK] and tags(w, index) == "{" * len(want)
    rw = RW.RowWalk(w, index)
    assert strings_of(RW.string_column(rw, (b"type",), False)) == [e["type"] for e in want]
    assert strings_of(RW.string_column(rw, (b"actor", b"login"), False)) == [e["actor"]["login"] for e in want]
    assert RW.select_rows(w, (b"type",))[2] == [NOT_OBJECT]

    doc = fixtures.load("citm_catalog")
    w, want = walk_of(doc), json.loads(doc)["performances"]
    offs, index, sts = RW.select_rows(w, (b"performances",))
    assert offs == [0, len(want)] and sts == [OK] and len(want) > 100
    rw = RW.RowWalk(w, index)
    assert RW.column(rw, (b"id",), CW.COL_INT) == ([p["id"] for p in want], [OK] * len(want))
    assert RW.column(rw, (b"eventId",), CW.COL_UINT) == ([p["eventId"] for p in want], [OK] * len(want))
    lo, vals, lst = RW.list_column(rw, (b"seatCategories",), CW.COL_INT)
    assert lst == [TYPE] * len(want) and vals == []  # (arrays of objects are no list of numbers)
