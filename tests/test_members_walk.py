"""CPU: the restated member rows of tests/members_walk.py (the checker of sjhip_unnest_members), pinned three ways: hand-written
documents whose parents hit every status, with the rows, the join back and the names written out by hand -- duplicate names, "" as
a name, escaped names, scalar and array parents, {} --; Python's json (object_pairs_hook=list: duplicates and order survive) as
the outside arbiter on the fixtures that keep a collection as a map: citm_catalog (events, areaNames, topicSubTopics) and
update-center (plugins); and THE PARITY CLAIM the device's tile pass rests on, asserted on every document these tests use: the tag
words at the rows' depth inside the OK parents' targets, in tape order, are key, value, key, value -- the odd ranks are exactly
the model's rows, and the even rank in front of each is a string tag two words in front of it."""
import json

import pytest

import column_walk as CW
import fixtures
import members_docs as D
import members_walk as MW
import rows_walk as RW
import unnest_walk as UW
from test_rows_walk import strings_of, tags, walk_of

OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)


def run_steps(w, steps):
    """the steps of a members_docs entry on the serial models -> [(step, depth of its rows, parents' RowWalk, result)]"""
    sel, depth, out = None, 0, []
    for kind, path in steps:
        rw = UW.record_rows(w) if sel is None else RW.RowWalk(w, sel[1])
        args = () if sel is None else (sel[0], sel[2])
        depth = (depth if sel is not None else 0) + len(path) + 1
        if kind == "select":
            assert sel is None
            res = RW.select_rows(w, path)
        elif kind == "unnest":
            res = UW.unnest_rows(rw, path, *args)
        else:
            res = MW.unnest_members(rw, path, *args)
        out.append(((kind, path), depth, rw, res))
        sel = res[:3]
    return out


def check_parity(w, steps):
    """-> the member rows the steps checked"""
    seen = 0
    for (kind, path), depth, rw, res in run_steps(w, steps):
        if kind != "members":
            continue
        starts = MW.member_starts(rw, path, depth)
        index, names = res[1], res[6]
        assert len(starts) == 2 * len(index)
        assert [i for i, _ in starts[1::2]] == index              # the odd ranks are exactly the rows
        for (ki, kt), (vi, _) in zip(starts[0::2], starts[1::2]):  # ... and the rank in front is the key: a string, two words in front
            assert kt == '"' and ki == vi - 2
        assert MW.names_of(w, index) == names
        seen += len(index)
    return seen


def test_every_parent_status():
    w = walk_of(D.STATUS_DOC, nd=True)
    offs, index, sts, poffs, parent, psts, names = run_steps(w, D.DOCS[0][3])[-1][3]
    assert (offs, sts, poffs, psts, parent, tags(w, index), names) == D.STATUS_WANT
    assert index == sorted(set(index)) and len(parent) == len(index) == poffs[-1] == offs[-1]
    # without a selection the parents are the records: "o" is an array, null, an array, an array
    res = MW.unnest_members(UW.record_rows(w), (b"o",))
    assert res[1] == [] and res[5] == [TYPE, NULL, TYPE, TYPE] and res[2] == [OK] * 4 and res[0] == [0] * 5


def test_kinds_of_parents_and_composition():
    w = walk_of(D.KINDS_DOC)
    base = RW.select_rows(w, ())
    res = MW.unnest_members(RW.RowWalk(w, base[1]), (), base[0], base[2])
    assert res[5] == [OK, OK, TYPE, TYPE, NULL, TYPE, OK, TYPE, OK] and res[6] == [b"a", b"b", b"k", b""]
    assert tags(w, res[1]) == "l{{{" and res[4] == [0, 0, 6, 8] and res[0] == [0, 4]
    res = MW.unnest_members(RW.RowWalk(w, base[1]), (b"k",), base[0], base[2])  # FindElement does not enter arrays; scalars are no objects
    assert res[5] == [NOT_FOUND, NOT_FOUND, NOT_OBJECT, NOT_OBJECT, NOT_OBJECT, NOT_OBJECT, OK, NOT_OBJECT, NOT_FOUND] and res[6] == [b"k"]
    w = walk_of(D.MAP_OF_MAPS)
    res = MW.unnest_members(UW.record_rows(w), (b"m",))
    assert res[6] == [b"a", b"b", b"c", b"d", b"e", b"a"] and tags(w, res[1]) == '{{{["{'
    res = MW.unnest_members(RW.RowWalk(w, res[1]), (), res[0], res[2])  # members of members: what lies deeper is not a row
    assert res[6] == [b"x", b"y", b"z", b"y"] and res[5] == [OK, OK, OK, TYPE, TYPE, OK] and res[4] == [0, 0, 2, 5]
    assert [CW.convert(w, i, CW.COL_INT) for i in res[1]] == [(OK, 1), (OK, 2), (TYPE, 0), (OK, 5)]
    w = walk_of(D.ARRAY_OF_OBJECTS)
    base = RW.select_rows(w, (b"items",))
    res = MW.unnest_members(RW.RowWalk(w, base[1]), (), base[0], base[2])
    assert res[6] == [b"id", b"name", b"t", b"id", b"id", b"id", b"o"] and res[3] == [0, 3, 3, 4, 4, 7] and res[5] == [OK, OK, OK, TYPE, OK]


def pairs_at(doc, *keys):
    """the first member named keys[0], keys[1], ... from the root, as json's list of (name, value) pairs"""
    v = json.loads(doc, object_pairs_hook=list)
    for k in keys:
        v = next(val for name, val in v if name == k)
    return v


def test_fixtures_against_json():
    doc = fixtures.load("citm_catalog")
    w = walk_of(doc)
    for key in ("events", "areaNames", "seatCategoryNames", "subTopicNames", "topicSubTopics"):
        want = pairs_at(doc, key)
        res = MW.unnest_members(UW.record_rows(w), (key.encode(),))
        assert res[5] == [OK] and res[0] == [0, len(want)] and len(want) > 3 and res[4] == [0] * len(want)
        assert res[6] == [name.encode() for name, _ in want]
        rows = RW.RowWalk(w, res[1])
        if key == "events":
            assert RW.column(rows, (b"id",), CW.COL_INT) == ([dict(v)["id"] for _, v in want], [OK] * len(want))
            assert [int(n) for n in res[6]] == [dict(v)["id"] for _, v in want]  # the map is keyed by the id
        elif key == "topicSubTopics":
            kids = UW.unnest_rows(rows, (), res[0], res[2])
            assert [CW.convert(w, i, CW.COL_INT)[1] for i in kids[1]] == [x for _, v in want for x in v]
            assert kids[4] == [p for p, (_, v) in enumerate(want) for _ in v]
        else:
            assert tags(w, res[1]) == '"' * len(want) and [w.string_at(i).decode() for i in res[1]] == [v for _, v in want]
    doc = fixtures.load("update-center")
    w = walk_of(doc)
    want = pairs_at(doc, "plugins")
    res = MW.unnest_members(UW.record_rows(w), (b"plugins",))
    assert len(want) > 500 and res[6] == [name.encode() for name, _ in want]
    assert strings_of(RW.string_column(RW.RowWalk(w, res[1]), (b"name",), False)) == [dict(v)["name"] for _, v in want]
    assert sum(n.startswith(b"git") for n in res[6]) == sum(name.startswith("git") for name, _ in want) > 3


def test_names_unescaped():
    w = walk_of(D.names_doc())
    res = MW.unnest_members(UW.record_rows(w), (b"m",))
    want = [name.encode() for name, _ in pairs_at(D.names_doc(), "m")]
    assert res[6] == want and [len(n) for n in want[:12]] == list(D.NAME_LENGTHS)
    assert b'a"b' in want and "é\n".encode() in want and want.count(b"dup") == 2 and b"\\" in want
    for copy in (True, False):
        assert MW.names_of(walk_of(D.names_doc(), copy=copy), res[1]) == want


@pytest.mark.parametrize("entry", D.DOCS, ids=[e[0] for e in D.DOCS])
def test_parity_of_the_starts(entry):
    name, doc, nd, steps = entry
    seen = check_parity(walk_of(doc, nd=nd), steps)
    assert seen > 0 or name in ("status records",)


def test_parity_on_the_fixtures():
    w = walk_of(fixtures.load("citm_catalog"))
    for key in (b"events", b"areaNames", b"topicSubTopics"):
        assert check_parity(w, [("members", (key,))]) > 3
    assert check_parity(w, [("members", (b"events",)), ("members", ())]) > 1000  # every field of every event
    assert check_parity(walk_of(fixtures.load("update-center")), [("members", (b"plugins",))]) > 500
    assert check_parity(walk_of(D.parking_lines(), nd=True), [("members", ())]) > 400
    assert check_parity(walk_of(D.sharded_lines(300), nd=True), [("members", (b"m",))]) > 300
