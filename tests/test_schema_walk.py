"""CPU: the restated row schema of tests/schema_walk.py (the checker of sjhip_row_schema), pinned two ways: hand-written documents
whose rows hit every status, with the names, first rows and counts written out by hand -- duplicate names inside one object, escaped
spellings of one name, "" as a name, one name with all eight types --; and Python's json as the outside arbiter
(object_pairs_hook: a list of (name, value) pairs, so duplicates and order survive; Python types mapped to the eight classes, an
integer told INT from UINT by its range, as the parser tells them) on twitter's statuses and their users, the events of
citm_catalog, the plugins of update-center, the parking-citations records and github_events."""
import json

import fixtures
import members_docs as D
import members_walk as MW
import rows_walk as RW
import schema_walk as SW
import unnest_walk as UW
from test_rows_walk import walk_of

OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)
N, S, I, U, F, B, O, A = range(8)  # the columns of counts: SJHIP_TYPE_* - 1


class Pairs(list):
    """a JSON object as json delivers it to object_pairs_hook: the list of its (name, value) pairs, told from a JSON array"""


def loads(doc):
    return json.loads(doc, object_pairs_hook=Pairs)


def type_of(v):
    if v is None:
        return SW.TYPE_NULL
    if isinstance(v, bool):
        return SW.TYPE_BOOL
    if isinstance(v, str):
        return SW.TYPE_STRING
    if isinstance(v, int):  # (no fraction, no exponent) int64 where it fits, then uint64, then a float
        return SW.TYPE_INT if -(1 << 63) <= v < (1 << 63) else (SW.TYPE_UINT if v < (1 << 64) else SW.TYPE_FLOAT)
    if isinstance(v, float):
        return SW.TYPE_FLOAT
    return SW.TYPE_OBJECT if isinstance(v, Pairs) else SW.TYPE_ARRAY


def json_object_at(v, path):
    """FindElement(path...) + Iter.Object on a value of loads() -> (the object's pairs, OK) or (None, status)"""
    for k, key in enumerate(path):
        if not isinstance(v, Pairs):
            return None, NOT_OBJECT
        hit = [val for name, val in v if name.encode() == key]
        if not hit:
            return None, NOT_FOUND
        v = hit[0]  # (the first member with the key wins at every level)
    if v is None:
        return None, NULL
    return (v, OK) if isinstance(v, Pairs) else (None, TYPE)


def json_schema(rows, path):
    status, names, first_row, counts, members = [0] * 6, [], [], [], 0
    for p, v in enumerate(rows):
        obj, st = json_object_at(v, path)
        status[st] += 1
        for name, val in obj or ():
            name = name.encode("utf-8", "surrogatepass")
            if name not in names:
                names.append(name)
                first_row.append(p)
                counts.append([0] * 8)
            counts[names.index(name)][type_of(val) - 1] += 1
            members += 1
    return len(rows), status, members, names, first_row, counts


def counts_of(**by_type):
    row = [0] * 8
    for k, n in by_type.items():
        row["NSIUFBOA".index(k)] = n
    return row


def test_every_status_duplicates_and_escapes():
    w = walk_of(D.STATUS_DOC, nd=True)
    rw = RW.RowWalk(w, RW.select_rows(w, (b"o",))[1])
    rows, status, members, names, first_row, counts = SW.row_schema(rw, (b"a",))
    assert (rows, members) == (11, 8) and status == [4, 1, 2, 3, 1, 0] and [OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL] == [0, 1, 2, 3, 4]
    assert names == [b"x", b"y", b"", b'a"b', "é\n".encode(), b"d"] and first_row == [0, 0, 8, 8, 8, 9]
    assert counts == [counts_of(I=1, A=1), counts_of(O=1), counts_of(B=1), counts_of(S=1), counts_of(N=1), counts_of(S=2)]
    # without a selection the rows are the records: "o" is an array, null, an array, an array
    assert SW.row_schema(UW.record_rows(w), (b"o",)) == (4, [0, 0, 0, 3, 1, 0], 0, [], [], [])
    # scalars and arrays as rows; an empty path: the row's own value
    w = walk_of(D.KINDS_DOC)
    rw = RW.RowWalk(w, RW.select_rows(w, ())[1])
    got = SW.row_schema(rw, ())
    assert got[:4] == (9, [4, 0, 0, 4, 1, 0], 4, [b"a", b"b", b"k", b""]) and got[4] == [0, 0, 6, 8]
    assert got[5] == [counts_of(I=1), counts_of(O=1), counts_of(O=1), counts_of(O=1)]
    assert SW.row_schema(rw, (b"k",))[1] == [1, 3, 5, 0, 0, 0]


def test_names_are_unescaped_bytes_and_types_follow_the_tag():
    doc = b'[{"\\u0061":1,"a":2.5,"A":3,"":4,"":null},{"a":"s","A":[]}]'
    w = walk_of(doc)
    got = SW.row_schema(RW.RowWalk(w, RW.select_rows(w, ())[1]), ())
    assert got == (2, [2, 0, 0, 0, 0, 0], 7, [b"a", b"A", b""], [0, 0, 0],
                   [counts_of(I=1, F=1, S=1), counts_of(I=1, A=1), counts_of(I=1, N=1)])
    doc = b'{"k":null,"k":"s","k":-1,"k":9223372036854775807,"k":9223372036854775808,"k":1e0,"k":true,"k":false,"k":{},"k":[]}'
    got = SW.row_schema(UW.record_rows(walk_of(doc)), ())
    assert got == (1, [1, 0, 0, 0, 0, 0], 10, [b"k"], [0], [[1, 1, 2, 1, 1, 2, 1, 1]])
    assert got == json_schema([loads(doc)], ())
    assert [SW.type_of_tag(t) for t in 'n"ludtf{['] == [1, 2, 3, 4, 5, 6, 6, 7, 8]


def check_against_json(w, rw, rows, paths):
    seen = 0
    for path in paths:
        got, want = SW.row_schema(rw, path), json_schema(rows, path)
        assert got == want, path
        assert sum(map(sum, got[5])) == got[2] and sum(got[1]) == got[0] == len(rows)
        seen += got[2]
    return seen


def test_fixtures_against_json():
    doc = fixtures.load("twitter")
    w = walk_of(doc)
    rows = dict(loads(doc))["statuses"]
    rw = RW.RowWalk(w, RW.select_rows(w, (b"statuses",))[1])
    assert check_against_json(w, rw, rows, [(), (b"user",), (b"entities",), (b"retweeted_status", b"user"), (b"geo",), (b"nope",)]) > 5000
    doc = fixtures.load("citm_catalog")
    w = walk_of(doc)
    rows = [v for _, v in dict(loads(doc))["events"]]
    rw = RW.RowWalk(w, MW.unnest_members(UW.record_rows(w), (b"events",))[1])
    assert len(rows) == 184 and check_against_json(w, rw, rows, [(), (b"name",)]) == 184 * len(rows[0])
    assert check_against_json(w, UW.record_rows(w), [loads(doc)], [(), (b"events",), (b"areaNames",), (b"topicSubTopics",)]) > 200
    doc = fixtures.load("update-center")
    w = walk_of(doc)
    rows = [v for _, v in dict(loads(doc))["plugins"]]
    rw = RW.RowWalk(w, MW.unnest_members(UW.record_rows(w), (b"plugins",))[1])
    assert len(rows) > 500 and check_against_json(w, rw, rows, [(), (b"developers",), (b"labels",)]) > 5000
    doc = D.parking_lines()
    w = walk_of(doc, nd=True)
    rows = [loads(line) for line in doc.split(b"\n")]
    assert check_against_json(w, UW.record_rows(w), rows, [(), (b"Make",)]) > 400 * 10
    doc = fixtures.load("github_events")
    w = walk_of(doc)
    rows = loads(doc)
    rw = RW.RowWalk(w, RW.select_rows(w, ())[1])
    assert check_against_json(w, rw, rows, [(), (b"payload",), (b"actor",), (b"repo",), (b"payload", b"commits")]) > 300


def test_the_member_documents():
    """the documents of the member-row tests: the schema of a step's parents counts exactly the rows unnest_members gives"""
    for name, doc, nd, steps in D.DOCS:
        w = walk_of(doc, nd=nd)
        sel = None
        for kind, path in steps:
            rw = UW.record_rows(w) if sel is None else RW.RowWalk(w, sel[1])
            args = () if sel is None else (sel[0], sel[2])
            if kind == "select":
                sel = RW.select_rows(w, path)
                continue
            if kind == "unnest":
                sel = UW.unnest_rows(rw, path, *args)[:3]
                continue
            res = MW.unnest_members(rw, path, *args)
            rows, status, members, names, first_row, counts = SW.row_schema(rw, path)
            assert rows == len(res[5]) and status == [res[5].count(s) for s in range(6)] and members == len(res[1]), name
            assert names == list(dict.fromkeys(res[6])) and first_row == [res[4][res[6].index(n)] for n in names], name
            assert [sum(c) for c in counts] == [res[6].count(n) for n in names], name
            sel = res[:3]
