"""GPU: the unnest (sjhip_unnest_rows / sjhip_fetch_row_parents) against the serial walk of tests/unnest_walk.py over the oracle's
parse -- the new selection as sjhip_fetch_rows returns it, the parents product, and every call that runs on rows on the new rows
-- and against Python's json where stated: on the fixtures with a second level, without a selection, on every parent status, on
scalar and array parents, on records owning 0 to 7 parents owning 0 to 7 children, with no parents and no rows at all, behind a
row predicate and behind an order (the depth of the rows carried through a narrowing), through the join back, at the seams of the
2048-word tape tile and of the scans, on a sharded result, and through the lifecycle.  Everything is compared exactly."""
import ctypes as C
import json
from collections import Counter

import numpy as np
import pytest

import fixtures
import group_walk as GW
import query_walk as Q
import rows_walk as RW
import unnest_walk as UW
import where_walk as WW
from test_gpu_aggregate import check_aggregates
from test_gpu_columns import oracle_walk
from test_gpu_filter_rows import check_filter
from test_gpu_group import check_group
from test_gpu_marshal_rows import check_marshal
from test_gpu_order import check_order
from test_gpu_parse import ctx  # noqa: F401
from test_gpu_rows import RAW, SEAM_COUNTS, TILE, check_queries
from test_gpu_tables import KINDS6
from test_gpu_where import check_where
from test_unnest_walk import STATUS_DOC, STATUS_WANT

pytestmark = pytest.mark.gpu

F, I, U, B, S, SC = KINDS6
OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)


def tags(w, index):
    return "".join(chr(int(w.t[int(i)]) >> 56) for i in index)


def select(ctx, w, path):
    sel = RW.select_rows(w, path)
    assert ctx.select_rows(path) == (len(sel[2]), len(sel[1])), path
    return sel


def check_unnest(ctx, w, sel, path):
    """unnest_rows on the selection in force (sel: the walker's copy of it, None without one) equals the walker: the counts, the
    new selection as fetch_rows delivers it, the parents product; -> the walker's result (its first three: the new selection)"""
    rw = UW.record_rows(w) if sel is None else RW.RowWalk(w, sel[1])
    want = UW.unnest_rows(rw, path) if sel is None else UW.unnest_rows(rw, path, sel[0], sel[2])
    offs, index, sts, poffs, parent, psts = want
    got = ctx.unnest_rows(path)
    assert got == (len(sts), len(psts), len(index)), (path, got, len(sts), len(psts), len(index))
    nr, npar, rows = got
    off, idx, st = ctx.fetch_rows(nr, rows)
    assert off.dtype == np.uint64 and idx.dtype == np.uint64 and st.dtype == np.uint8
    assert off.tolist() == offs and st.tolist() == sts, path
    assert np.array_equal(idx, np.array(index, dtype=np.uint64)), path
    po, pa, ps = ctx.fetch_row_parents(npar, rows)
    assert po.dtype == np.uint64 and pa.dtype == np.uint64 and ps.dtype == np.uint8
    assert po.tolist() == poffs and ps.tolist() == psts, path
    assert np.array_equal(pa, np.array(parent, dtype=np.uint64)), path
    return want


def check_consumers(ctx, w, sel, paths, where, order, copy=True):
    """every consumer of a selection on the new rows: the battery of tests/test_gpu_rows.py, marshal_rows, filter_rows, then
    where_path and order_path (which narrow), against the row walkers on RowWalk(new index)"""
    rw = RW.RowWalk(w, sel[1])
    check_queries(ctx, rw, paths)
    check_marshal(ctx, w, sel[1])
    if copy:
        check_filter(ctx, w, sel[1])
    sel = check_where(ctx, w, sel, *where)
    check_queries(ctx, RW.RowWalk(w, sel[1]), paths[:1])
    got, want = check_order(ctx, w, sel, *order)
    return want.selection


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_fixtures(ctx, copy):
    doc = fixtures.load("twitter")
    w, statuses = oracle_walk(doc, False, copy), json.loads(doc)["statuses"]
    ctx.parse(doc, copy_strings=copy, key_flags=True)
    sel = check_unnest(ctx, w, select(ctx, w, (b"statuses",)), (b"entities", b"hashtags"))
    assert len(sel[1]) == 8 and sel[5] == [OK] * 100
    got, want = check_group(ctx, RW.RowWalk(w, sel[1]), (b"text",), GW.COL_STRING)
    count = Counter(h["text"].encode() for s in statuses for h in s["entities"]["hashtags"])
    assert got.groups == 7 and dict(zip(got.keys, got.group_rows.tolist())) == dict(count)
    check_consumers(ctx, w, sel[:3], [(b"text",), (b"indices",)], ((b"text",), WW.OP_PREFIX_STRING, b""), ((b"indices",), I, False, 3), copy)

    sel = check_unnest(ctx, w, select(ctx, w, (b"statuses",)), (b"entities", b"user_mentions"))
    assert len(sel[1]) == 87
    sel = check_unnest(ctx, w, sel[:3], (b"indices",))
    assert len(sel[1]) == 174 and tags(w, sel[1]) == "l" * 174
    total, per = check_aggregates(ctx, RW.RowWalk(w, sel[1]), sel[0], (), I)
    assert total.count == 174 and total.sum == sum(x for s in statuses for m in s["entities"]["user_mentions"] for x in m["indices"])
    check_consumers(ctx, w, sel[:3], [(b"a",)], ((), WW.OP_GT_INT, 20), ((), I, True, 50), copy)

    doc = fixtures.load("citm_catalog")
    w, perf = oracle_walk(doc, False, copy), json.loads(doc)["performances"]
    ctx.parse(doc, copy_strings=copy, key_flags=True)
    sel = check_unnest(ctx, w, select(ctx, w, (b"performances",)), (b"prices",))
    assert len(sel[1]) == 907
    sel = check_unnest(ctx, w, select(ctx, w, (b"performances",)), (b"seatCategories",))
    sel = check_unnest(ctx, w, sel[:3], (b"areas",))
    areas = [a["areaId"] for p in perf for c in p["seatCategories"] for a in c["areas"]]
    assert len(sel[1]) == 8685 and ctx.extract_path((b"areaId",), I)[0].tolist() == areas
    check_consumers(ctx, w, sel[:3], [(b"areaId",), (b"blockIds",)], ((b"areaId",), WW.OP_GE_INT, sorted(areas)[4000]),
                    ((b"areaId",), U, True, 100), copy)

    doc = fixtures.load("github_events")
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy, key_flags=True)
    sel = check_unnest(ctx, w, select(ctx, w, ()), (b"payload", b"commits"))
    assert len(sel[1]) == 16 and sel[5].count(NOT_FOUND) == 17 and sel[5].count(OK) == 13
    check_consumers(ctx, w, sel[:3], [(b"sha",), (b"author", b"name"), (b"distinct",)], ((b"distinct",), Q.OP_EQ_BOOL, True),
                    ((b"author", b"name"), I, False, 5), copy)
    ctx.select_records()


# ---- without a selection, statuses, kinds of parents -----------------------------------------------------------------------------------
def test_without_a_selection(ctx):
    w = oracle_walk(STATUS_DOC, True, True)
    ctx.parse(STATUS_DOC, ndjson=True)
    for path in ((b"o",), (), (b"nope",)):
        ctx.select_records()
        want = check_unnest(ctx, w, None, path)
        nr, rows = ctx.select_rows(path)
        off, idx, st = ctx.fetch_rows(nr, rows)
        assert (off.tolist(), idx.tolist()) == (want[0], want[1]) and (off.tolist(), st.tolist()) == (want[3], want[5])
        assert want[2] == [OK] * 4
    ctx.select_records()


def test_every_parent_status(ctx):
    w = oracle_walk(STATUS_DOC, True, True)
    ctx.parse(STATUS_DOC, ndjson=True)
    want = check_unnest(ctx, w, select(ctx, w, (b"o",)), (b"a",))
    assert (want[0], want[2], want[3], want[5], want[4], tags(w, want[1])) == STATUS_WANT
    assert sorted(set(want[5])) == [OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL]
    ctx.select_records()


def test_parent_row_kinds(ctx):
    doc = b'[[1,2],[3],[],7,null,[[4],5],"s",{"k":[6]}]'
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    base = select(ctx, w, ())
    sel = check_unnest(ctx, w, base, ())  # arrays as parents, no keys: lists of lists
    assert tags(w, sel[1]) == "lll[l" and sel[5] == [OK, OK, OK, TYPE, NULL, OK, TYPE, TYPE]
    sel = check_unnest(ctx, w, sel[:3], ())  # scalars as parents, no keys; the one array among them has a row
    assert tags(w, sel[1]) == "l" and sel[5] == [TYPE, TYPE, TYPE, OK, TYPE]
    sel = check_unnest(ctx, w, sel[:3], (b"k",))  # a scalar parent with keys
    assert sel[1] == [] and sel[5] == [NOT_OBJECT]
    select(ctx, w, ())
    sel = check_unnest(ctx, w, base, (b"k",))  # arrays and scalars as parents with keys: FindElement does not enter arrays
    assert sel[5] == [NOT_OBJECT] * 7 + [OK] and tags(w, sel[1]) == "l"
    ctx.select_records()


def nested_lines(n_records):
    """record r owns (r * 5) % 8 parents -- the elements of "items" --, parent j of it owns (j * 3 + r * 2) % 8 children in "t\""""
    lines = []
    for r in range(n_records):
        items = []
        for j in range((r * 5) % 8):
            kids = ['{"v":%d,"t":[%d]}' % (r * 8 + c, c) if c % 3 == 0 else ("[%d,[%d]]" % (c, r) if c % 3 == 1 else str(r * 100 + c))
                    for c in range((j * 3 + r * 2) % 8)]
            items.append('{"id":%d,"t":[%s],"u":[9,[9]]}' % (r * 8 + j, ",".join(kids)))
        lines.append('{"k":%d,"items":[%s]}' % (r, ",".join(items)))
    return "\n".join(lines).encode()


def check_0_to_7(ctx, n_records=300):
    doc = nested_lines(n_records)
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    sel = check_unnest(ctx, w, select(ctx, w, (b"items",)), (b"t",))
    assert len(sel[5]) > 1000 and len(sel[1]) > 3000 and set(np.diff(sel[3]).tolist()) == set(range(8))
    check_queries(ctx, RW.RowWalk(w, sel[1]), [(b"v",), (b"t",)])
    sel = check_unnest(ctx, w, sel[:3], (b"t",))  # the objects among the children have one more level
    assert len(sel[1]) > 300 and tags(w, sel[1]) == "l" * len(sel[1])
    ctx.select_records()


def test_records_owning_0_to_7_parents_owning_0_to_7_children(ctx):
    check_0_to_7(ctx)


def test_no_parents_and_no_rows(ctx):
    doc = b'{"items":[]}\n{"items":null}\n{"x":[1,2]}\n[{"items":[1]}]'
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    sel = check_unnest(ctx, w, select(ctx, w, (b"items",)), (b"t",))  # no parents at all
    assert (sel[1], sel[3], sel[4], sel[5]) == ([], [0], [], []) and sel[2] == [OK, NULL, NOT_FOUND, NOT_OBJECT]
    assert len(ctx.find_path(b"x")) == 0
    sel = check_unnest(ctx, w, sel[:3], ())  # ... and again on the empty selection
    assert sel[1] == [] and sel[2] == [OK, NULL, NOT_FOUND, NOT_OBJECT]
    sel = check_unnest(ctx, w, select(ctx, w, (b"x",)), (b"t",))  # parents, no rows
    assert sel[1] == [] and sel[3] == [0, 0, 0] and sel[5] == [NOT_OBJECT, NOT_OBJECT]
    assert ctx.count_where_path((b"x",), ctx.OP_EXISTS) == 0
    ctx.select_records()
    assert len(ctx.find_path(b"x")) == 4


# ---- composition: the depth of the rows carried through a narrowing --------------------------------------------------------------------
def test_behind_a_predicate_and_behind_an_order(ctx):
    doc = nested_lines(120)
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    base = select(ctx, w, (b"items",))
    sel = check_where(ctx, w, base, (b"id",), WW.OP_GE_INT, 200)
    assert 0 < len(sel[1]) < len(base[1])
    sel = check_unnest(ctx, w, sel, (b"t",))
    assert len(sel[1]) > 100
    check_queries(ctx, RW.RowWalk(w, sel[1]), [(b"v",)])
    select(ctx, w, (b"items",))
    got, want = check_order(ctx, w, base, (b"id",), I, True, 100)
    sel = check_unnest(ctx, w, want.selection, (b"t",))
    assert len(sel[5]) == 100 and len(sel[1]) > 100
    ctx.select_records()
    sel = check_where(ctx, w, None, (b"k",), WW.OP_GE_INT, 60)  # a selection a predicate created: the root values, depth 0
    sel = check_unnest(ctx, w, sel, (b"items",))
    sel = check_unnest(ctx, w, sel[:3], (b"t",))
    assert len(sel[1]) > 500
    ctx.select_records()


def test_the_join_back(ctx):
    doc = fixtures.load("twitter")
    statuses = json.loads(doc)["statuses"]
    ctx.parse(doc)
    ctx.select_rows((b"statuses",))
    ids = ctx.extract_path((b"id",), I)[0]  # a parent column, fetched before the call
    nr, npar, rows = ctx.unnest_rows((b"entities", b"user_mentions"))
    assert (nr, npar, rows) == (1, 100, 87)
    po, parent, ps = ctx.fetch_row_parents(npar, rows)
    names = ctx.extract_path_strings((b"screen_name",))
    want = [(s["id"], m["screen_name"].encode()) for s in statuses for m in s["entities"]["user_mentions"]]
    assert list(zip(np.take(ids, parent).tolist(), [names[1][names[0][k]:names[0][k + 1]] for k in range(rows)])) == want
    assert np.array_equal(np.repeat(np.arange(100, dtype=np.uint64), np.diff(po).astype(np.int64)), parent)
    ctx.select_records()


# ---- the seams of the 2048-word tile -----------------------------------------------------------------------------------------------------
BIG = 2300  # numbers in the long parent: 4600 words, so it spans three tiles wherever it starts
SEAM_PARENTS = [
    '{"s":%d,"t":[true,%d,{"a":[1,{"t":[5]}],"t":[6]},[[1],2],"x",null,%d,%d],"u":%d}' % (RAW["["], RAW["{"], RAW["]"], RAW["["], RAW["]"]),
    '{"t":[]}', "7", '{"t":[%s]}' % ",".join(str(k) for k in range(BIG)),
    '{"s":[%d,%d],"t":[%d,{"t":[1]},false],"u":{"t":[%d]}}' % (RAW["{"], RAW["["], RAW["]"], RAW["["]), '{"t":[[],{}]}']


def seam_doc(first, parents=SEAM_PARENTS):
    """one document whose first child -- the `true` of the first parent's "t" -- lies at tape word `first`:
    r { "p" [ pad ] "items" [ { "s" number "t" [ true ..."""
    extra = first - 17
    assert extra >= 0
    pad = ["0"] * (extra // 2) + ["true"] * (extra % 2)
    return ('{"p":[%s],"items":[%s]}' % (",".join(pad), ",".join(parents))).encode()


def check_tile_seam(ctx, first):
    doc = seam_doc(first)
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = check_unnest(ctx, w, select(ctx, w, (b"items",)), (b"t",))
    assert sel[1][0] == first and tags(w, sel[1][:8]) == 'tl{["nll' and sel[3] == [0, 8, 8, 8, 8 + BIG, 11 + BIG, 13 + BIG]
    if first in (TILE - 1, TILE, TILE + 1):
        check_queries(ctx, RW.RowWalk(w, sel[1]), [(b"a",), (b"t",)])
    sel = check_unnest(ctx, w, sel[:3], (b"t",))  # a further level: {"a":..,"t":[6]} and {"t":[1]}
    assert tags(w, sel[1]) == "ll"
    ctx.select_records()


@pytest.mark.parametrize("first", list(range(TILE - 14, TILE + 2)))
def test_children_at_the_tile_boundary(ctx, first):
    """first = 2048: the target '[' is the last word of a tile and its first element the first word of the next; the other
    alignments put the parent's '{' and the child's start on either side of the cut, the numbers' raw words -- which look like
    '[', '{' and ']', inside the target range and just outside it on both sides -- at the cut in turn; the long parent spans three
    tiles in every one of them"""
    check_tile_seam(ctx, first)


def check_anchor_retry(ctx):
    """runs of integers whose tag AND raw word look like two-word tags (l), as pad and as children: a tile finds no anchor among
    the 64 words in front of it and the global anchors decide"""
    lit = str(RAW["l"])
    parents = ['{"t":[%s]}' % ",".join([lit] * 700), '{"s":[%s],"t":[{"t":[%s]},%s]}' % (",".join([lit] * 1300), lit, lit), '{"t":[%s]}' % lit]
    doc = ('{"p":[%s],"items":[%s]}' % (",".join([lit] * 1100), ",".join(parents))).encode()
    w = oracle_walk(doc, False, True)
    run = [i for i in range(TILE - 70, TILE) if chr(w.t[i] >> 56) not in '"lud']
    assert run == [] and len(w.t) > 3 * TILE
    ctx.parse(doc)
    sel = check_unnest(ctx, w, select(ctx, w, (b"items",)), (b"t",))
    assert sel[3] == [0, 700, 702, 703]
    sel = check_unnest(ctx, w, sel[:3], (b"t",))
    assert len(sel[1]) == 1
    ctx.select_records()


def test_anchor_window_defeated(ctx):
    check_anchor_retry(ctx)


# ---- the seams of the scans ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SEAM_COUNTS)
def test_parent_and_row_counts_at_the_seams(ctx, n):
    doc = ('{"items":[%s]}' % ",".join('{"t":[%d]}' % r if r % 7 else '{"t":[{"v":%d}]}' % r for r in range(n))).encode()  # n parents, n rows
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = check_unnest(ctx, w, select(ctx, w, (b"items",)), (b"t",))
    assert len(sel[5]) == n and len(sel[1]) == n
    doc = ('{"items":[{"t":[%s]},{"t":[1]},{"x":0}]}' % ",".join(str(r) if r % 5 else '{"v":[%d]}' % r for r in range(n - 1))).encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = check_unnest(ctx, w, select(ctx, w, (b"items",)), (b"t",))  # 3 parents, n rows
    assert len(sel[5]) == 3 and len(sel[1]) == n and sel[3] == [0, n - 1, n, n]
    assert len(ctx.find_path(b"v")) == n
    ctx.select_records()


# ---- a sharded result ------------------------------------------------------------------------------------------------------------------
def test_sharded_result_equals_whole():
    import sjhip
    lines = []
    for k in range(9000):
        items = ['{"id":%d,"tags":[%s],"pad":"%s"}' % (k * 3 + j, ",".join('"t%d"' % (k + c) for c in range((k + j * 3) % 8)), "x" * 60)
                 for j in range(3)]
        lines.append('{"order":%d,"items":[%s]}' % (k, ",".join(items)))
    doc = "\n".join(lines).encode()
    assert len(doc) > (2 << 20)
    one = sjhip.Context(0)
    one.parse(doc, ndjson=True)
    one.select_rows((b"items",))
    want = one.unnest_rows((b"tags",))
    want_rows, want_parents = one.fetch_rows(want[0], want[2]), one.fetch_row_parents(want[1], want[2])
    with fixtures.nd_shard_limits(2 << 20, 1 << 20):
        many = sjhip.Context(0)
        many.parse(doc, ndjson=True)
    assert many.select_rows((b"items",)) == (9000, 27000)
    assert many.unnest_rows((b"tags",)) == want and want[:2] == (9000, 27000) and want[2] > 80000
    for a, b in zip(many.fetch_rows(want[0], want[2]), want_rows):
        assert np.array_equal(a, b)
    for a, b in zip(many.fetch_row_parents(want[1], want[2]), want_parents):  # both rebasings: offsets by rows, parent by parents
        assert np.array_equal(a, b)
    po, parent, ps = want_parents
    assert np.array_equal(np.repeat(np.arange(27000, dtype=np.uint64), np.diff(po).astype(np.int64)), parent)
    kept = one.where_path((), one.OP_EQ_STRING, b"t77")  # a consumer of the new rows: the tag "t77" lies in a handful of lines
    assert many.where_path((), many.OP_EQ_STRING, b"t77") == kept and 0 < kept[1] < 30
    for a, b in zip(many.fetch_rows(*kept), one.fetch_rows(*kept)):
        assert np.array_equal(a, b)
    many.select_records()
    many.close()
    one.close()


# ---- lifecycle ---------------------------------------------------------------------------------------------------------------------------
def test_lifecycle(ctx):
    import sjhip
    fresh = sjhip.Context(0)
    doc = b'{"o":1,"items":[{"t":[1,2]},{"t":[]},{"t":[3]}]}\n{"o":2,"items":[{"t":null}]}'
    fresh.parse(doc, ndjson=True)
    with pytest.raises(sjhip.ParseError) as e:
        fresh.fetch_row_parents(4, 3)
    assert e.value.code == 5 and "no row parents on the device" in str(e.value)
    assert fresh.select_rows((b"items",)) == (2, 4)
    base = fresh.device_bytes()
    assert fresh.unnest_rows((b"t",)) == (2, 4, 3) and fresh.device_bytes() > base  # the arena of the parents
    want = fresh.fetch_row_parents(4, 3)
    assert want[0].tolist() == [0, 2, 2, 3, 3] and want[1].tolist() == [0, 0, 2] and want[2].tolist() == [OK, OK, OK, NULL]
    assert fresh.fetch_rows(2, 3)[0].tolist() == [0, 3, 3]
    rows_before = fresh.fetch_rows(2, 3)

    def same_parents():
        for a, b in zip(fresh.fetch_row_parents(4, 3), want):
            assert np.array_equal(a, b)
    # SJHIP_ERR_ARG touches nothing: a bad path, a null size pointer
    L, h = sjhip.lib(), fresh._h
    lens, a, b, c = (C.c_uint32 * 1)(1), C.c_size_t(77), C.c_size_t(77), C.c_size_t(77)
    with pytest.raises(sjhip.ParseError) as e:
        fresh.unnest_rows((b"k",) * 17)
    assert e.value.code == 5
    for args in [(None, C.byref(b), C.byref(c)), (C.byref(a), None, C.byref(c)), (C.byref(a), C.byref(b), None)]:
        assert L.sjhip_unnest_rows(h, b"t", lens, 1, *args) == 5
        assert b"null size pointer" in L.sjhip_last_error(h)
    assert L.sjhip_unnest_rows(h, None, None, 1, C.byref(a), C.byref(b), C.byref(c)) == 5
    same_parents()
    for x, y in zip(fresh.fetch_rows(2, 3), rows_before):
        assert np.array_equal(x, y)
    # any destination of the fetch may be null
    only = np.zeros(3, np.uint64)
    assert L.sjhip_fetch_row_parents(h, None, only.ctypes.data, None) == 0 and only.tolist() == [0, 0, 2]
    assert L.sjhip_fetch_row_parents(h, None, None, None) == 0
    # the parents survive every change of the selection and every other product
    fresh.select_records()
    same_parents()
    assert fresh.where_path((b"o",), fresh.OP_GE_INT, 2) == (2, 1)
    fresh.extract_table([((b"o",), I), ((b"items",), SC)])
    fresh.extract_path_strings((b"o",), cvt=True)
    fresh.marshal_json()
    fresh.serialize()
    fresh.select_rows((b"items",))
    fresh.order_path((b"t",), I)
    same_parents()
    # a parse, a failed parse, trim drop them; a call without a result is refused
    for drop in (lambda: fresh.parse(b'{"items":[1]}', ndjson=True), lambda: pytest.raises(sjhip.ParseError, fresh.parse, b'{"s":'),
                 fresh.trim):
        fresh.parse(doc, ndjson=True)
        fresh.select_rows((b"items",))
        fresh.unnest_rows((b"t",))
        drop()
        with pytest.raises(sjhip.ParseError) as e:
            fresh.fetch_row_parents(4, 3)
        assert "no row parents on the device" in str(e.value)
    assert fresh.device_bytes() == 0  # (after trim: the arena went with the others)
    fresh.parse(doc, ndjson=True)
    fresh.select_rows((b"items",))
    before = fresh.device_bytes()
    fresh.unnest_rows((b"t",))
    assert fresh.device_bytes() > before  # ... it is allocated again and counted, and trim returns it
    fresh.trim()
    assert fresh.device_bytes() == 0
    with pytest.raises(sjhip.ParseError) as e:
        fresh.unnest_rows((b"t",))
    assert e.value.code == 5
    fresh.close()
