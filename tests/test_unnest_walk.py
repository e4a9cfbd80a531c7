"""CPU: the restated unnest of tests/unnest_walk.py (the checker of sjhip_unnest_rows), pinned two ways: a hand-written document
whose parent rows hit every status, with the rows and the join back written out by hand -- lists of lists, scalar parents, nested
elements that must not become rows --, and Python's json as the outside arbiter on the fixtures with a second level: twitter
(statuses -> entities.hashtags / entities.user_mentions -> indices), citm_catalog (performances -> prices / seatCategories ->
areas), github_events (the root array -> payload.commits)."""
import json

import column_walk as CW
import fixtures
import rows_walk as RW
import unnest_walk as UW
from test_rows_walk import strings_of, tags, walk_of

OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)

# one NDJSON input whose parent rows -- the elements of "o" -- hit every status under the path ("a",)
# (tests/test_gpu_unnest.py runs the device on it)
STATUS_DOC = b"\n".join([
    b'{"o":[{"a":[1,{"a":[7]},[2,3]]},{"x":1},{"a":null},{"a":"s"},5,[{"a":[9]}],{"a":[]},{"a":{"a":[1]}},{"b":2,"a":[true]}]}',
    b'{"o":null}',
    b'{"o":[]}',
    b'{"o":[{"a":["x","y"],"a":[0]},{"a":{"b":1},"a":[4]}]}',  # duplicate keys: the first wins
])
STATUS_PARENTS = [OK, NOT_FOUND, NULL, TYPE, NOT_OBJECT, NOT_OBJECT, OK, TYPE, OK, OK, TYPE]
STATUS_WANT = ([0, 4, 4, 4, 6], [OK, NULL, OK, OK],                       # the records: new row offsets, statuses kept
               [0, 3, 3, 3, 3, 3, 3, 3, 3, 4, 6, 6], STATUS_PARENTS,       # the parents: offsets over the new rows, statuses
               [0, 0, 0, 8, 9, 9], 'l{[t""')                               # the new rows: their parent, their tag


def unnest_chain(w, first, *more):
    """select_rows(first), then unnest_rows for every further path -> the last unnest's result (or the selection's, as a 3-tuple)"""
    offs, index, sts = RW.select_rows(w, first)
    out = (offs, index, sts)
    for path in more:
        out = UW.unnest_rows(RW.RowWalk(w, index), path, offs, sts)
        offs, index, sts = out[:3]
    return out


def test_every_parent_status():
    w = walk_of(STATUS_DOC, nd=True)
    offs, index, sts, poffs, parent, psts = unnest_chain(w, (b"o",), (b"a",))
    assert (offs, sts, poffs, psts, parent, tags(w, index)) == STATUS_WANT
    assert index == sorted(set(index)) and len(parent) == len(index) == poffs[-1] == offs[-1]
    for p in range(len(psts)):
        assert parent[poffs[p]:poffs[p + 1]] == [p] * (poffs[p + 1] - poffs[p])


def test_lists_of_lists_and_scalar_parents():
    w = walk_of(b'[[1,2],[3],[],7,null,[[4],5]]')
    offs, index, sts, poffs, parent, psts = unnest_chain(w, (), ())
    assert (offs, sts) == ([0, 5], [OK]) and psts == [OK, OK, OK, TYPE, NULL, OK]
    assert poffs == [0, 2, 3, 3, 3, 3, 5] and parent == [0, 0, 1, 5, 5] and tags(w, index) == "lll[l"
    assert [CW.convert(w, i, CW.COL_INT) for i in index] == [(OK, 1), (OK, 2), (OK, 3), (TYPE, 0), (OK, 5)]
    # a third level: only the array among the rows has elements; scalar parents with keys are NOT_OBJECT
    out = UW.unnest_rows(RW.RowWalk(w, index), (), offs, sts)
    assert out[0] == [0, 1] and out[3:] == ([0, 0, 0, 0, 1, 1], [3], [TYPE, TYPE, TYPE, OK, TYPE]) and tags(w, out[1]) == "l"
    assert UW.unnest_rows(RW.RowWalk(w, index), (b"k",), offs, sts)[5] == [NOT_OBJECT] * 5
    # arrays as parents with keys: FindElement does not descend into arrays
    assert unnest_chain(w, (), (b"k",))[5] == [NOT_OBJECT] * 6


def test_without_a_selection_it_is_the_row_selection():
    w = walk_of(STATUS_DOC, nd=True)
    for path in ((b"o",), (), (b"nope",)):
        offs, index, sts = RW.select_rows(w, path)
        got = UW.unnest_rows(UW.record_rows(w), path)
        assert got[:2] == (offs, index) and got[2] == [OK] * 4          # the statuses of the records: all OK
        assert got[3] == offs and got[5] == sts                         # ... the parents carry select_rows' offsets and statuses
        assert got[4] == [r for r in range(4) for _ in range(offs[r], offs[r + 1])]


def test_fixtures_against_json():
    doc = fixtures.load("twitter")
    w, want = walk_of(doc), json.loads(doc)["statuses"]
    offs, index, sts, poffs, parent, psts = unnest_chain(w, (b"statuses",), (b"entities", b"hashtags"))
    owners = [k for k, s in enumerate(want) for _ in s["entities"]["hashtags"]]
    assert (offs, sts, psts) == ([0, 8], [OK], [OK] * 100) and len(index) == 8 and len(set(owners)) == 7
    assert parent == owners and sum(s["entities"]["hashtags"] == [] for s in want) == 93
    texts = strings_of(RW.string_column(RW.RowWalk(w, index), (b"text",), False))
    assert texts == [h["text"] for s in want for h in s["entities"]["hashtags"]] and len(set(texts)) == 7
    offs, index, sts, poffs, parent, psts = unnest_chain(w, (b"statuses",), (b"entities", b"user_mentions"))
    assert len(index) == 87 and parent == [k for k, s in enumerate(want) for _ in s["entities"]["user_mentions"]]
    assert strings_of(RW.string_column(RW.RowWalk(w, index), (b"screen_name",), False)) == \
        [m["screen_name"] for s in want for m in s["entities"]["user_mentions"]]
    mentions = [m for s in want for m in s["entities"]["user_mentions"]]
    offs, index, sts, poffs, parent, psts = UW.unnest_rows(RW.RowWalk(w, index), (b"indices",), offs, sts)
    assert len(index) == 174 and offs == [0, 174] and parent == [k for k, m in enumerate(mentions) for _ in m["indices"]]
    assert [CW.convert(w, i, CW.COL_INT) for i in index] == [(OK, x) for m in mentions for x in m["indices"]]

    doc = fixtures.load("citm_catalog")
    w, want = walk_of(doc), json.loads(doc)["performances"]
    assert len(want) == 243
    offs, index, sts, poffs, parent, psts = unnest_chain(w, (b"performances",), (b"prices",))
    assert len(index) == 907 and parent == [k for k, p in enumerate(want) for _ in p["prices"]]
    offs, index, sts, poffs, parent, psts = unnest_chain(w, (b"performances",), (b"seatCategories",), (b"areas",))
    areas = [a for p in want for c in p["seatCategories"] for a in c["areas"]]
    assert len(index) == 8685 == len(areas) and offs == [0, 8685]
    assert RW.column(RW.RowWalk(w, index), (b"areaId",), CW.COL_INT) == ([a["areaId"] for a in areas], [OK] * 8685)

    doc = fixtures.load("github_events")
    w, want = walk_of(doc), json.loads(doc)
    offs, index, sts, poffs, parent, psts = unnest_chain(w, (), (b"payload", b"commits"))
    commits = [(k, c) for k, e in enumerate(want) for c in e["payload"].get("commits", [])]
    assert len(want) == 30 and len(index) == 16 and psts.count(NOT_FOUND) == 17 and psts.count(OK) == 13
    assert parent == [k for k, _ in commits] and len(set(parent)) == 13
    assert strings_of(RW.string_column(RW.RowWalk(w, index), (b"sha",), False)) == [c["sha"] for _, c in commits]
