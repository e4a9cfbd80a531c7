"""GPU: the member rows (sjhip_unnest_members / sjhip_extract_row_names / sjhip_where_row_names) against the serial walk of
tests/members_walk.py over the oracle's parse -- the new selection as sjhip_fetch_rows returns it, the parents product, the names,
and every call that runs on rows on the new rows -- and against Python's json where stated: on the fixtures that keep a collection
as a map, at the seams of thread, wave and tile with the key and the value of a member on either side of a cut and odd tiles
handing their parity on, on what must not be counted, on raw words that look like tags with the global anchors in force, on names
of every length around the copy switch, through the name predicate, in composition with the row selection and the unnest, with
nothing to find, on a sharded result, and through the lifecycle.  Everything is compared exactly."""
import ctypes as C
import json
from collections import Counter

import numpy as np
import pytest

import fixtures
import group_walk as GW
import members_docs as D
import members_walk as MW
import rows_walk as RW
import unnest_walk as UW
import where_walk as WW
from test_gpu_columns import oracle_walk
from test_gpu_group import check_group
from test_gpu_marshal_rows import check_marshal
from test_gpu_order import check_order
from test_gpu_parse import ctx  # noqa: F401
from test_gpu_rows import RAW, SEAM_COUNTS, TILE, check_queries
from test_gpu_tables import KINDS6
from test_gpu_unnest import check_consumers, check_unnest, select, tags
from test_gpu_where import check_where
from test_members_walk import pairs_at

pytestmark = pytest.mark.gpu

F, I, U, B, S, SC = KINDS6
OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)
REFUSED = "the rows in force are not object members (sjhip_extract_row_names follows sjhip_unnest_members)"


def test_the_documents_are_the_seams_they_claim():
    assert (RAW, SEAM_COUNTS, TILE) == (D.RAW, D.SEAM_COUNTS, D.TILE)


def check_names(ctx, w, index):
    """extract_row_names on the member selection in force, whose row index is `index`, equals the names read from the tape"""
    want = MW.names_of(w, index)
    assert ctx.extract_row_names(fetch=False) == (len(want), sum(len(n) for n in want))
    off, data, st = ctx.extract_row_names()
    assert off.dtype == np.uint64 and st.dtype == np.uint8 and st.tolist() == [OK] * len(want)
    assert off.tolist() == np.cumsum([0] + [len(n) for n in want]).tolist() and data == b"".join(want)
    return want


def check_members(ctx, w, sel, path):
    """unnest_members on the selection in force (sel: the walker's copy of it, None without one) equals the walker: the counts,
    the new selection as fetch_rows delivers it, the parents product, the names; -> the walker's result"""
    rw = UW.record_rows(w) if sel is None else RW.RowWalk(w, sel[1])
    want = MW.unnest_members(rw, path) if sel is None else MW.unnest_members(rw, path, sel[0], sel[2])
    offs, index, sts, poffs, parent, psts, names = want
    got = ctx.unnest_members(path)
    assert got == (len(sts), len(psts), len(index)), (path, got, len(sts), len(psts), len(index))
    nr, npar, rows = got
    off, idx, st = ctx.fetch_rows(nr, rows)
    assert off.tolist() == offs and st.tolist() == sts, path
    assert np.array_equal(idx, np.array(index, dtype=np.uint64)), path
    po, pa, ps = ctx.fetch_row_parents(npar, rows)
    assert po.dtype == np.uint64 and pa.dtype == np.uint64 and ps.dtype == np.uint8
    assert po.tolist() == poffs and ps.tolist() == psts, path
    assert np.array_equal(pa, np.array(parent, dtype=np.uint64)), path
    assert check_names(ctx, w, index) == names
    return want


def check_where_names(ctx, w, sel, op, value, negate=False):
    """where_row_names on the member selection `sel` in force keeps what the host keeps on the names; -> the new selection"""
    names = MW.names_of(w, sel[1])
    hit = [(n == value if op == ctx.OP_EQ_STRING else n.startswith(value)) != negate for n in names]
    index = [i for i, h in zip(sel[1], hit) if h]
    pre = np.cumsum([0] + hit).tolist()
    offs = [pre[int(o)] for o in sel[0]]
    got = ctx.where_row_names(op, value, negate=negate)
    assert got == (len(sel[2]), len(index)), (op, value, negate, got, len(index))
    off, idx, st = ctx.fetch_rows(*got)
    assert off.tolist() == offs and idx.tolist() == index and st.tolist() == list(sel[2])
    return offs, index, list(sel[2])


def run_steps(ctx, w, steps):
    sel = None
    for kind, path in steps:
        if kind == "select":
            sel = select(ctx, w, path)
        elif kind == "unnest":
            sel = check_unnest(ctx, w, sel if sel is None else sel[:3], path)
        else:
            sel = check_members(ctx, w, sel if sel is None else sel[:3], path)
    return sel


def check_doc(ctx, name, copy=True):
    name, doc, nd, steps = next(e for e in D.DOCS if e[0] == name)
    w = oracle_walk(doc, nd, copy)
    ctx.parse(doc, ndjson=nd, copy_strings=copy, key_flags=True)
    sel = run_steps(ctx, w, steps)
    return w, sel


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def check_fixtures(ctx, copy):
    doc = fixtures.load("citm_catalog")
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy, key_flags=True)
    events = pairs_at(doc, "events")
    sel = check_members(ctx, w, None, (b"events",))
    assert sel[6] == [n.encode() for n, _ in events] and len(events) == 184
    ids = [dict(v)["id"] for _, v in events]
    assert ctx.extract_path((b"id",), I)[0].tolist() == ids
    kept = check_where_names(ctx, w, sel[:3], ctx.OP_EQ_STRING, b"138586341")  # the event whose id is 138586341
    assert len(kept[1]) == 1 and ctx.extract_path((b"id",), I)[0].tolist() == [138586341]
    ctx.select_records()
    sel = check_members(ctx, w, None, (b"events",))
    check_consumers(ctx, w, sel[:3], [(b"id",), (b"name",), (b"subTopicIds",)], ((b"id",), WW.OP_GE_INT, sorted(ids)[90]),
                    ((b"id",), I, True, 20), copy)
    ctx.select_records()
    names = pairs_at(doc, "areaNames")
    sel = check_members(ctx, w, None, (b"areaNames",))  # string rows: the consumers take the empty path
    assert tags(w, sel[1]) == '"' * len(names) and sel[6] == [n.encode() for n, _ in names]
    got, want = check_group(ctx, RW.RowWalk(w, sel[1]), (), GW.COL_STRING)
    assert dict(zip(got.keys, got.group_rows.tolist())) == dict(Counter(v.encode() for _, v in names))
    check_marshal(ctx, w, sel[1])
    kept = check_where(ctx, w, sel[:3], (), WW.OP_PREFIX_STRING, b"Arri")
    assert 0 < len(kept[1]) < len(names) and check_names(ctx, w, kept[1]) == [n.encode() for n, v in names if v.startswith("Arri")]
    ctx.select_records()
    sub = pairs_at(doc, "topicSubTopics")
    sel = check_members(ctx, w, None, (b"topicSubTopics",))  # the values are arrays: one more level through the unnest
    kids = check_unnest(ctx, w, sel[:3], ())
    assert kids[4] == [p for p, (_, v) in enumerate(sub) for _ in v]
    total = ctx.aggregate_path((), I)
    assert total.count == len(kids[1]) and total.sum == sum(x for _, v in sub for x in v)
    ctx.select_records()

    doc = fixtures.load("update-center")
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy, key_flags=True)
    plugins = pairs_at(doc, "plugins")
    sel = check_members(ctx, w, None, (b"plugins",))
    assert sel[6] == [n.encode() for n, _ in plugins]
    got, want = check_group(ctx, RW.RowWalk(w, sel[1]), (b"buildDate",), GW.COL_STRING)
    assert dict(zip(got.keys, got.group_rows.tolist())) == dict(Counter(dict(v)["buildDate"].encode() for _, v in plugins))
    kept = check_where_names(ctx, w, sel[:3], ctx.OP_PREFIX_STRING, b"git")  # the plugins whose name begins with git
    assert check_names(ctx, w, kept[1]) == [n.encode() for n, _ in plugins if n.startswith("git")] and len(kept[1]) > 3
    check_queries(ctx, RW.RowWalk(w, kept[1]), [(b"name",), (b"dependencies",)])
    ctx.select_records()

    doc = D.parking_lines()
    w = oracle_walk(doc, True, copy)
    ctx.parse(doc, ndjson=True, copy_strings=copy, key_flags=True)
    sel = check_members(ctx, w, None, ())  # every field of every line
    lines = [json.loads(line) for line in doc.split(b"\n")]
    assert len(sel[1]) == sum(len(x) for x in lines) and sel[3] == np.cumsum([0] + [len(x) for x in lines]).tolist()
    kept = check_where_names(ctx, w, sel[:3], ctx.OP_EQ_STRING, b"Make")
    got, want = check_group(ctx, RW.RowWalk(w, kept[1]), (), GW.COL_STRING)
    assert dict(zip(got.keys, got.group_rows.tolist())) == dict(Counter(x["Make"].encode() for x in lines if isinstance(x.get("Make"), str)))
    ctx.select_records()


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_fixtures(ctx, copy):
    check_fixtures(ctx, copy)


# ---- the seams of thread, wave and tile ----------------------------------------------------------------------------------------------
def check_tile_seam(ctx, key_at):
    w, sel = check_doc(ctx, "seam %d" % key_at)
    assert sel[1][0] == key_at + 2 and len(sel[1]) == 3060 and sel[6][:2] == [b"m0", b"m1"]
    starts = [i for v in sel[1] for i in (v - 2, v)]
    per_tile = Counter(i // TILE for i in starts)
    assert len(per_tile) >= 4 and sum(n % 2 for n in per_tile.values()) >= 3  # odd tiles hand their parity on
    if key_at in (TILE - 1, TILE - 2):
        check_queries(ctx, RW.RowWalk(w, sel[1]), [(b"m1",), (b"x", b"y")])
    kids = check_members(ctx, w, sel[:3], ())  # a further level: the members of the object values, and of {}
    assert len(kids[1]) == 2 * sum(1 for j in range(60) if j % 7 == 3) and set(kids[6]) == {b"m1", b"x"}
    ctx.select_records()


@pytest.mark.parametrize("key_at", D.SEAM_KEYS)
def test_members_at_the_tile_boundary(ctx, key_at):
    """key_at = TILE - 1: the key's tag word is the last of a tile and its length word the first of the next; TILE - 2: the key
    ends a tile and its value begins the next; the members behind put every other cut of thread (8 words) and wave (512) in turn"""
    check_tile_seam(ctx, key_at)


@pytest.mark.parametrize("n", SEAM_COUNTS)
def test_member_counts_at_the_seams(ctx, n):
    w, sel = check_doc(ctx, "one object %d" % n)
    assert len(sel[1]) == n and sel[5] == [OK]
    w, sel = check_doc(ctx, "spread %d" % n)
    assert len(sel[1]) == n and set(np.diff(sel[3]).tolist()) <= set(range(8))
    ctx.select_records()


# ---- what must not be counted ------------------------------------------------------------------------------------------------------------
def test_every_parent_status(ctx):
    w, sel = check_doc(ctx, "status")
    assert (sel[0], sel[2], sel[3], sel[5], sel[4], tags(w, sel[1]), sel[6]) == D.STATUS_WANT
    assert sorted(set(sel[5])) == [OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL]
    w, sel = check_doc(ctx, "status records")
    assert sel[1] == [] and sel[5] == [TYPE, NULL, TYPE, TYPE]
    ctx.select_records()


def test_parent_row_kinds(ctx):
    w, sel = check_doc(ctx, "kinds")
    assert sel[5] == [OK, OK, TYPE, TYPE, NULL, TYPE, OK, TYPE, OK] and sel[6] == [b"a", b"b", b"k", b""]
    w, sel = check_doc(ctx, "kinds keyed")
    assert sel[6] == [b"z"] and tags(w, sel[1]) == "["
    ctx.select_records()


def check_0_to_7(ctx):
    w, sel = check_doc(ctx, "0 to 7")
    assert len(sel[5]) > 1000 and len(sel[1]) > 2000 and set(np.diff(sel[3]).tolist()) == set(range(8))
    assert {NOT_FOUND, NULL, TYPE, OK} == set(sel[5])
    check_queries(ctx, RW.RowWalk(w, sel[1]), [(b"m1",), (b"x", b"y")])
    ctx.select_records()


def test_records_owning_0_to_7_parents_owning_0_to_7_members(ctx):
    check_0_to_7(ctx)


# ---- the anchor rule ------------------------------------------------------------------------------------------------------------------------
def check_anchor_retry(ctx):
    doc = D.anchor_doc()
    w = oracle_walk(doc, False, True)
    run = [i for i in range(TILE - 70, TILE) if chr(w.t[i] >> 56) not in '"lud']
    assert run == [] and len(w.t) > 2 * TILE  # more than 64 words that look like two-word tags in front of a tile boundary
    w, sel = check_doc(ctx, "anchor")
    assert len(sel[1]) == 902 and tags(w, sel[1]) == "l" * 900 + "{["
    assert ctx.aggregate_path((), I).count == 900
    assert ctx.count_where_path((b"r1",), ctx.OP_EQ_INT, RAW["l"]) == 1
    ctx.select_records()


def test_raw_words_and_the_global_anchors(ctx):
    check_anchor_retry(ctx)


# ---- names --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_names(ctx, copy):
    w, sel = check_doc(ctx, "names", copy)
    names = sel[6]
    assert [len(n) for n in names[:12]] == list(D.NAME_LENGTHS) and b'a"b' in names and "é\n".encode() in names and names.count(b"dup") == 2
    base = sel[:3]
    kept = check_where(ctx, w, base, (), WW.OP_GE_INT, 5)  # after a where_path
    assert check_names(ctx, w, kept[1]) == names[5:]
    got, want = check_order(ctx, w, kept, (), I, True, 7)  # after an order with a limit
    assert check_names(ctx, w, want.selection[1]) == names[-7:]
    ctx.select_records()
    run_steps(ctx, w, [("members", (b"m",))])
    kept = check_where_names(ctx, w, base, ctx.OP_PREFIX_STRING, b"n" * 32)  # after where_row_names: 32, 33, 63, 64, 65, 512, 33
    assert check_names(ctx, w, kept[1]) == [n for n in names if n.startswith(b"n" * 32)] and len(kept[1]) == 7
    kept = check_where_names(ctx, w, kept, ctx.OP_EQ_STRING, b"n" * 33)
    assert len(kept[1]) == 2
    ctx.select_records()


def test_where_row_names(ctx):
    import sjhip
    w, sel = check_doc(ctx, "names")
    base, n = sel[:3], len(sel[1])

    def again():
        ctx.select_records()
        run_steps(ctx, w, [("members", (b"m",))])
    for op, value, kept in [(ctx.OP_EQ_STRING, b"dup", 2), (ctx.OP_EQ_STRING, b"", 1), (ctx.OP_EQ_STRING, b'a"b', 1), (ctx.OP_EQ_STRING, b"nope", 0),
                            (ctx.OP_EQ_STRING, "é\n".encode(), 1), (ctx.OP_PREFIX_STRING, b"", n), (ctx.OP_PREFIX_STRING, b"gi", 3),
                            (ctx.OP_PREFIX_STRING, b"git", 2), (ctx.OP_PREFIX_STRING, b"n" * 512, 1), (ctx.OP_PREFIX_STRING, b"n" * 513, 0)]:
        for negate in (False, True):
            got = check_where_names(ctx, w, base, op, value, negate)
            assert len(got[1]) == (n - kept if negate else kept), (op, value, negate)
            again()
    before = ctx.fetch_rows(1, n)
    for op in (ctx.OP_EXISTS, ctx.OP_EQ_INT, ctx.OP_EQ_BOOL, ctx.OP_IS_NULL, ctx.OP_LT_INT, ctx.OP_GE_FLOAT, 20, -1):  # the refused operators
        with pytest.raises(sjhip.ParseError) as e:
            ctx.where_row_names(op, b"12345678")
        assert e.value.code == 5 and "sjhip_where_row_names" in str(e.value)
    L = sjhip.lib()
    a, b = C.c_size_t(7), C.c_size_t(7)
    assert L.sjhip_where_row_names(ctx._h, ctx.OP_EQ_STRING, b"x", 1, 2, C.byref(a), C.byref(b)) == 5  # an unknown flag
    assert L.sjhip_where_row_names(ctx._h, ctx.OP_EQ_STRING, b"x", 1, 0, None, C.byref(b)) == 5
    assert L.sjhip_where_row_names(ctx._h, ctx.OP_EQ_STRING, b"x" * 2000, 2000, 0, C.byref(a), C.byref(b)) == 5  # where_path's limit
    for x, y in zip(ctx.fetch_rows(1, n), before):
        assert np.array_equal(x, y)
    assert check_names(ctx, w, base[1]) == sel[6]
    ctx.select_records()


def test_names_need_member_rows(ctx):
    import sjhip
    doc = b'{"items":[{"a":{"x":1}},{"a":{"y":[2,3]}}]}'
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)

    def refused(rows):
        col = ctx.extract_path_strings((b"items",), cvt=True)  # a string column: a refused call leaves it
        for call in (ctx.extract_row_names, lambda: ctx.where_row_names(ctx.OP_EQ_STRING, b"x")):
            with pytest.raises(sjhip.ParseError) as e:
                call()
            assert e.value.code == 5 and REFUSED in str(e.value)
        got = ctx.fetch_path_strings(len(col[2]), len(col[1]))
        assert got[1] == col[1] and got[0].tolist() == col[0].tolist()
        if rows is not None:
            assert ctx.fetch_rows(1, len(rows))[1].tolist() == rows
        else:
            with pytest.raises(sjhip.ParseError):
                ctx.fetch_rows(1, 1)
    refused(None)                                    # without a selection
    sel = select(ctx, w, (b"items",))
    refused(sel[1])                                  # after select_rows
    sel = check_members(ctx, w, sel, (b"a",))
    assert sel[6] == [b"x", b"y"]
    kids = check_unnest(ctx, w, sel[:3], ())
    refused(kids[1])                                 # after unnest_rows, on the rows it left
    ctx.select_records()
    kept = check_where(ctx, w, None, (b"items",), ctx.OP_EXISTS)
    refused(kept[1])                                 # a selection a predicate created
    ctx.select_records()
    check_members(ctx, w, None, ())
    ctx.parse(doc)
    refused(None)                                    # ... and after a parse
    ctx.select_records()


# ---- composition ---------------------------------------------------------------------------------------------------------------------------
def test_composition(ctx):
    w, sel = check_doc(ctx, "map of maps")  # unnest_members twice
    assert sel[6] == [b"x", b"y", b"z", b"y"] and sel[5] == [OK, OK, OK, TYPE, TYPE, OK]
    w, sel = check_doc(ctx, "root object")
    assert sel[6] == [b"m"]
    w, sel = check_doc(ctx, "array of objects")  # select_rows, then every field of each
    assert sel[6] == [b"id", b"name", b"t", b"id", b"id", b"id", b"o"] and sel[5] == [OK, OK, OK, TYPE, OK]
    # the parents product and row_index through a later narrowing: parent numbers stay those of the selection the call found
    ctx.select_records()
    select(ctx, w, (b"items",))
    assert ctx.unnest_members(()) == (1, 5, 7)
    before, parents = ctx.fetch_rows(1, 7), ctx.fetch_row_parents(5, 7)
    kept = ctx.where_row_names(ctx.OP_EQ_STRING, b"id")
    assert kept == (1, 4)
    idx = ctx.fetch_rows(*kept)[1]
    assert idx.tolist() == [v for v, n in zip(before[1].tolist(), sel[6]) if n == b"id"]
    for a, b in zip(ctx.fetch_row_parents(5, 7), parents):
        assert np.array_equal(a, b)
    assert parents[1][np.searchsorted(before[1], idx)].tolist() == [0, 2, 4, 4]
    assert ctx.aggregate_path((), I).sum == 10
    ctx.select_records()


# ---- nothing to find ---------------------------------------------------------------------------------------------------------------------
def check_empty(ctx):
    doc = b'{"m":{}}\n{"m":null}\n{"x":{"a":1}}\n[{"m":{"a":1}}]'
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    sel = check_members(ctx, w, None, (b"m",))  # parents, no rows
    assert sel[1] == [] and sel[5] == [OK, NULL, NOT_FOUND, NOT_OBJECT] and sel[3] == [0] * 5
    assert ctx.where_row_names(ctx.OP_PREFIX_STRING, b"") == (4, 0)
    sel = check_members(ctx, w, sel[:3], ())  # no parents at all, on the empty member selection
    assert (sel[1], sel[3], sel[4], sel[5]) == ([], [0], [], []) and sel[2] == [OK] * 4
    assert ctx.extract_row_names(fetch=False) == (0, 0) and ctx.where_row_names(ctx.OP_EQ_STRING, b"a", negate=True) == (4, 0)
    ctx.select_records()
    sel = check_members(ctx, w, None, (b"x",))
    assert sel[6] == [b"a"] and sel[3] == [0, 0, 0, 1, 1]
    ctx.select_records()


def test_no_parents_and_no_rows(ctx):
    check_empty(ctx)


# ---- a sharded result ------------------------------------------------------------------------------------------------------------------
def test_sharded_result_equals_whole():
    import sjhip
    doc = D.sharded_lines()
    assert len(doc) > (2 << 20)
    one = sjhip.Context(0)
    one.parse(doc, ndjson=True)
    want = one.unnest_members((b"m",))
    want_rows, want_parents, want_names = one.fetch_rows(want[0], want[2]), one.fetch_row_parents(want[1], want[2]), one.extract_row_names()
    w = oracle_walk(doc, True, True)
    model = MW.unnest_members(UW.record_rows(w), (b"m",))
    assert want == (9000, 9000, len(model[1])) and want_rows[1].tolist() == model[1] and want[2] > 30000
    with fixtures.nd_shard_limits(2 << 20, 1 << 20):
        many = sjhip.Context(0)
        many.parse(doc, ndjson=True)
    assert many.unnest_members((b"m",)) == want
    for a, b in zip(many.fetch_rows(want[0], want[2]), want_rows):
        assert np.array_equal(a, b)
    for a, b in zip(many.fetch_row_parents(want[1], want[2]), want_parents):
        assert np.array_equal(a, b)
    got = many.extract_row_names()  # the joined fetch of the column
    assert got[1] == want_names[1] == b"".join(model[6]) and np.array_equal(got[0], want_names[0])
    kept = one.where_row_names(one.OP_PREFIX_STRING, b"m77")
    assert many.where_row_names(many.OP_PREFIX_STRING, b"m77") == kept and kept[1] == sum(n.startswith(b"m77") for n in model[6]) > 5
    for a, b in zip(many.fetch_rows(*kept), one.fetch_rows(*kept)):
        assert np.array_equal(a, b)
    assert many.extract_row_names()[1] == one.extract_row_names()[1]
    many.select_records()
    many.close()
    one.close()


# ---- lifecycle ---------------------------------------------------------------------------------------------------------------------------
def test_lifecycle():
    import sjhip
    fresh = sjhip.Context(0)
    doc = b'{"o":1,"m":{"a":1,"b":[2],"a":{"c":3}}}\n{"o":2,"m":null}'
    fresh.parse(doc, ndjson=True)
    with pytest.raises(sjhip.ParseError) as e:
        fresh.fetch_row_parents(2, 3)
    assert "no row parents on the device" in str(e.value)
    base = fresh.device_bytes()
    assert fresh.unnest_members((b"m",)) == (2, 2, 3) and fresh.device_bytes() > base  # the arena of the parents
    want = fresh.fetch_row_parents(2, 3)
    assert want[0].tolist() == [0, 3, 3] and want[1].tolist() == [0, 0, 0] and want[2].tolist() == [OK, NULL]
    rows_before = fresh.fetch_rows(2, 3)
    assert fresh.extract_row_names()[1] == b"aba"
    # SJHIP_ERR_ARG touches nothing: a bad path, a null size pointer
    L, h = sjhip.lib(), fresh._h
    lens, a, b, c = (C.c_uint32 * 1)(1), C.c_size_t(77), C.c_size_t(77), C.c_size_t(77)
    with pytest.raises(sjhip.ParseError):
        fresh.unnest_members((b"k",) * 17)
    for args in [(None, C.byref(b), C.byref(c)), (C.byref(a), None, C.byref(c)), (C.byref(a), C.byref(b), None)]:
        assert L.sjhip_unnest_members(h, b"t", lens, 1, *args) == 5
        assert b"sjhip_unnest_members: a null size pointer" in L.sjhip_last_error(h)
    assert L.sjhip_extract_row_names(h, None, C.byref(b)) == 5
    for x, y in zip(fresh.fetch_row_parents(2, 3), want):
        assert np.array_equal(x, y)
    for x, y in zip(fresh.fetch_rows(2, 3), rows_before):
        assert np.array_equal(x, y)
    assert fresh.fetch_path_strings(3, 3)[1] == b"aba"
    # the parents survive the selection and the other products; a parse and trim drop them, and the member selection with them
    fresh.select_records()
    fresh.extract_path_strings((b"o",), cvt=True)
    fresh.marshal_json()
    for x, y in zip(fresh.fetch_row_parents(2, 3), want):
        assert np.array_equal(x, y)
    for drop in (lambda: fresh.parse(b'{"m":{"a":1}}', ndjson=True), fresh.trim):
        fresh.parse(doc, ndjson=True)
        fresh.unnest_members((b"m",))
        drop()
        with pytest.raises(sjhip.ParseError) as e:
            fresh.fetch_row_parents(2, 3)
        assert "no row parents on the device" in str(e.value)
        with pytest.raises(sjhip.ParseError) as e:
            fresh.extract_row_names()
        assert e.value.code == 5
    assert fresh.device_bytes() == 0
    fresh.close()
