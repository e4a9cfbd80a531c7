"""GPU: row predicates (sjhip_where_path) against the serial restatement of tests/where_walk.py over the oracle's parse: what
fetch_rows delivers after a predicate, count_where_path of the same operator, and every call that runs on rows -- the battery of
tests/test_gpu_rows.py -- on the narrowed selection; on the fixtures, on random records with every operator, at the seams of the
wave (64), the block (256) and the scan tile (1024), on the empty path, at the number edges, with no rows kept, through the
lifecycle and on a sharded result in which whole shards keep nothing."""
import json
import struct

import numpy as np
import pytest

import column_walk as CW
import fixtures
import query_walk as Q
import rows_walk as RW
import table_walk as TW
import where_walk as WW
from test_gpu_columns import RANDOM_PATHS, oracle_walk, random_nd
from test_gpu_parse import ctx  # noqa: F401
from test_gpu_rows import check_queries, wrapped_random
from test_gpu_tables import KINDS6, same_column

pytestmark = pytest.mark.gpu

F, I, U, B, S, SC = KINDS6
OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)
# a value for every operator (the EDGES and STRINGS of tests/test_gpu_columns.py hold elements on both sides of each)
WANT = {Q.OP_EXISTS: None, Q.OP_EQ_STRING: b"HOND", Q.OP_EQ_INT: 1, Q.OP_EQ_UINT: 0, Q.OP_EQ_FLOAT: 0.0, Q.OP_EQ_BOOL: True,
        Q.OP_IS_NULL: None, WW.OP_PREFIX_STRING: b"a"}
for _op in WW.ORDER_OPS:
    WANT[_op] = {CW.COL_INT: 1, CW.COL_UINT: 1 << 63, CW.COL_FLOAT: 0.0}[WW.KIND_OF[_op]]


def check_where(ctx, w, sel, path, op, want=None, negate=False):
    """where_path on the selection in force (sel: the walker's, None without one) equals the walker, and count_where_path of the
    same operator counts the rows kept; -> the walker's new selection"""
    rows_before = len(sel[1]) if sel is not None else len(w.records())
    count = ctx.count_where_path(path, op, want) if len(path) else None  # (the count takes no empty path)
    want_off, want_idx, want_st = WW.where(w, sel, path, op, want, negate)
    nr, rows = ctx.where_path(path, op, want, negate=negate)
    assert (nr, rows) == (len(want_st), len(want_idx)), (path, op, want, negate, nr, rows)
    if count is not None:
        assert count == (rows_before - rows if negate else rows), (path, op, want, negate)
    off, idx, st = ctx.fetch_rows(nr, rows)
    assert off.dtype == np.uint64 and idx.dtype == np.uint64 and st.dtype == np.uint8
    assert st.tolist() == want_st and off.tolist() == want_off, (path, op, want, negate)
    assert np.array_equal(idx, np.array(want_idx, dtype=np.uint64)), (path, op, want, negate)
    return want_off, want_idx, want_st


# ---- parity, in both copy modes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_parity_on_items(ctx, copy):
    doc = wrapped_random(11, 700)
    w = oracle_walk(doc, True, copy)
    ctx.parse(doc, ndjson=True, copy_strings=copy)
    sel = RW.select_rows(w, (b"items",))
    assert ctx.select_rows((b"items",)) == (len(sel[2]), 700)
    sel = check_where(ctx, w, sel, (b"a",), Q.OP_EXISTS)
    assert 100 < len(sel[1]) < 700 and sel[0] != list(range(len(sel[0])))
    check_queries(ctx, RW.RowWalk(w, sel[1]), RANDOM_PATHS[:6], keys=[b"a", b"", b"c"],
                  eq=[(ctx.OP_EQ_STRING, (b"a",), b"HOND"), (ctx.OP_EQ_INT, (b"b",), 1)])
    sel = check_where(ctx, w, sel, (b"b",), Q.OP_IS_NULL, negate=True)  # a second call: the conjunction
    check_queries(ctx, RW.RowWalk(w, sel[1]), RANDOM_PATHS[:3])
    ctx.select_records()


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_parity_on_records(ctx, copy):
    doc = random_nd(11, 700)
    w = oracle_walk(doc, True, copy)
    ctx.parse(doc, ndjson=True, copy_strings=copy)
    sel = check_where(ctx, w, None, (b"a",), Q.OP_EXISTS)  # without a selection: it creates one, a row per matching record
    assert 100 < len(sel[1]) < 700 and sel[2] == [OK] * 700
    check_queries(ctx, RW.RowWalk(w, sel[1]), RANDOM_PATHS[:6], keys=[b"a", b"", b"c"], eq=[(ctx.OP_EQ_STRING, (b"a",), b"HOND")])
    ctx.select_records()
    assert len(ctx.find_path(b"a")) == 700


# ---- documents --------------------------------------------------------------------------------------------------------------------
def test_twitter_conjunction(ctx):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = RW.select_rows(w, (b"statuses",))
    ctx.select_rows((b"statuses",))
    sel = check_where(ctx, w, sel, (b"lang",), Q.OP_EQ_STRING, b"ja")
    sel = check_where(ctx, w, sel, (b"retweet_count",), WW.OP_GE_INT, 1)
    want = [s for s in json.loads(doc)["statuses"] if s["lang"] == "ja" and s["retweet_count"] >= 1]
    assert 0 < len(want) == len(sel[1]) < 100
    assert ctx.extract_path((b"id",), I)[0].tolist() == [s["id"] for s in want]
    off, data, st = ctx.extract_path_strings((b"user", b"screen_name"))
    assert [data[off[k]:off[k + 1]].decode() for k in range(len(want))] == [s["user"]["screen_name"] for s in want]
    ctx.select_records()


def test_github_events_prefix(ctx):
    doc = fixtures.load("github_events")
    w = oracle_walk(doc, False, True)
    events = json.loads(doc)
    for negate in (False, True):
        ctx.parse(doc)
        sel = RW.select_rows(w, ())
        ctx.select_rows(())
        sel = check_where(ctx, w, sel, (b"type",), WW.OP_PREFIX_STRING, b"Push", negate=negate)
        want = [e for e in events if e["type"].startswith("Push") != negate]
        assert 0 < len(want) == len(sel[1]) < len(events)
        off, data, st = ctx.extract_path_strings((b"id",))
        assert [data[off[k]:off[k + 1]].decode() for k in range(len(want))] == [e["id"] for e in want]
    ctx.select_records()


@pytest.mark.parametrize("wrapped", [False, True], ids=["records", "items"])
def test_every_operator_on_random_records(ctx, wrapped):
    doc = wrapped_random(7, 300) if wrapped else random_nd(7, 300)
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    base = RW.select_rows(w, (b"items",)) if wrapped else None
    kept = set()
    for op in WW.ALL_OPS:
        for k, path in enumerate(RANDOM_PATHS):
            if wrapped:
                ctx.select_rows((b"items",))
            else:
                ctx.select_records()
            sel = check_where(ctx, w, base, path, op, WANT[op], negate=(k + op) % 3 == 0)
            if len(sel[1]) not in (0, 300):
                kept.add(op)
    assert kept == set(WW.ALL_OPS), sorted(set(WW.ALL_OPS) - kept)  # every operator told rows apart somewhere
    ctx.select_records()


# ---- the seams of the wave, the block and the scan tile -------------------------------------------------------------------------
SEAM_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)


def seam_rows(n):
    """row r of n: its number, its parity, and a mark on the rows 1023 and 1024 -- the two sides of the scan tile's seam"""
    return ['{"v":%d,"p":%d,"m":%d}' % (r, r % 2, r in (1023, 1024)) for r in range(n)]


def check_seams(ctx, w, base, reselect, n):
    """predicates that keep every row, no row, only the first, only the last, every second, and exactly the rows 1023 and 1024, and
    their negations, each on the selection `base` (None: the records) put back in force by reselect()"""
    for path, op, want, kept in [((b"v",), WW.OP_GE_INT, 0, n), ((b"v",), WW.OP_LT_INT, 0, 0), ((b"v",), WW.OP_LE_INT, 0, 1),
                                 ((b"v",), WW.OP_GE_UINT, n - 1, 1), ((b"p",), Q.OP_EQ_UINT, 1, n // 2),
                                 ((b"m",), WW.OP_GT_FLOAT, 0.5, max(0, min(n, 1025) - 1023))]:
        for negate in (False, True):
            reselect()
            sel = check_where(ctx, w, base, path, op, want, negate)
            assert len(sel[1]) == (n - kept if negate else kept), (n, path, op, negate)
    ctx.select_records()


@pytest.mark.parametrize("n", SEAM_COUNTS)
def test_record_counts_at_the_seams(ctx, n):
    doc = "\n".join(seam_rows(n)).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    check_seams(ctx, w, None, ctx.select_records, n)


@pytest.mark.parametrize("n", SEAM_COUNTS)
def test_row_counts_at_the_seams(ctx, n):
    doc = ("[" + ",".join(seam_rows(n)) + "]").encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    base = RW.select_rows(w, ())
    assert len(base[1]) == n
    check_seams(ctx, w, base, lambda: ctx.select_rows(()), n)


@pytest.mark.parametrize("n", (257, 1025, 2049))
def test_records_owning_0_to_7_rows(ctx, n):
    rows, lines, at, k = seam_rows(n), [], 0, 0
    while at < n:
        take = (k * 5) % 8
        lines.append('{"k":%d,"items":[%s]}' % (k, ",".join(rows[at:at + take])))
        at += take
        k += 1
    doc = "\n".join(lines).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    base = RW.select_rows(w, (b"items",))
    assert len(base[1]) == n and base[0] != list(range(len(base[0])))
    check_seams(ctx, w, base, lambda: ctx.select_rows((b"items",)), n)


# ---- the empty path, the edges, no rows -------------------------------------------------------------------------------------------
def test_empty_path_on_scalar_rows(ctx):
    doc = b'[3,"a",null,7.5,-2]'
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = RW.select_rows(w, ())
    for negate, tags in ((False, "ld"), (True, '"nl')):
        ctx.select_rows(())
        got = check_where(ctx, w, sel, (), WW.OP_GT_FLOAT, 0.0, negate)
        assert "".join(chr(w.t[i] >> 56) for i in got[1]) == tags
    ctx.select_records()
    got = check_where(ctx, w, None, (), Q.OP_EXISTS)  # without a selection: the root value of the record
    assert got[1] == [1]
    ctx.select_records()


def test_number_edges(ctx):
    texts = ["9223372036854775808.0", "18446744073709551616.0", "-0.0", "9223372036854775808", "18446744073709551615",
             "-9223372036854775808.0", "9223372036854777856.0", "18446744073709555712.0", "1.5", "-1", "0", "null", '"1"']
    doc = "\n".join('{"v":%s}' % t for t in texts).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    wants = {CW.COL_INT: [0, -(1 << 63), (1 << 63) - 1, 1], CW.COL_UINT: [0, 1 << 63, (1 << 64) - 1, 1],
             CW.COL_FLOAT: [0.0, -0.0, 2.0 ** 63, 2.0 ** 64, float("nan")]}
    for op in WW.ORDER_OPS:
        for want in wants[WW.KIND_OF[op]]:
            for negate in (False, True):
                ctx.select_records()
                check_where(ctx, w, None, (b"v",), op, want, negate)
    # 2^63 as a float is MinInt64 under *_INT, 2^64 is 0 under *_UINT, -0.0 is not below 0.0, a u above MaxInt64 is no int64
    ctx.select_records()
    assert check_where(ctx, w, None, (b"v",), WW.OP_LT_INT, 0)[0][:6] == [0, 1, 1, 1, 1, 1]
    ctx.select_records()
    assert check_where(ctx, w, None, (b"v",), WW.OP_LE_UINT, 0)[0][:4] == [0, 0, 1, 2]
    ctx.select_records()
    assert check_where(ctx, w, None, (b"v",), WW.OP_LT_FLOAT, 0.0)[0][:4] == [0, 0, 0, 0]
    ctx.select_records()


def test_no_rows_kept(ctx):
    doc = random_nd(3, 200)
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    want_table = ctx.extract_table([((b"a",), SC)])
    sel = check_where(ctx, w, None, (b"nope",), Q.OP_EXISTS)
    assert sel == ([0] * 201, [], [OK] * 200)
    assert len(ctx.find_path(b"a")) == 0 and ctx.count_where_path((b"a",), ctx.OP_EXISTS) == 0
    assert ctx.project_keys([b"a", b"b"]).shape == (0, 2)
    for kind in (F, I, U, B):
        vals, st = ctx.extract_path((b"a",), kind)
        assert len(vals) == 0 and len(st) == 0
    off, data, st = ctx.extract_path_strings((b"a",), cvt=True)
    assert off.tolist() == [0] and data == b"" and len(st) == 0
    loff, vals, lst = ctx.extract_path_list((b"a",), I)
    assert loff.tolist() == [0] and len(vals) == 0 and len(lst) == 0
    (vals, st), (off, data, st2) = ctx.extract_table([((b"a",), I), ((b"a",), S)])
    assert len(vals) == 0 and len(st) == 0 and off.tolist() == [0] and data == b"" and len(st2) == 0
    assert check_where(ctx, w, sel, (b"a",), Q.OP_EXISTS) == sel  # a second predicate on the empty selection
    assert check_where(ctx, w, sel, (b"a",), Q.OP_EXISTS, negate=True) == sel
    ctx.select_records()
    same_column(SC, ctx.extract_table([((b"a",), SC)])[0], want_table[0], "records again")


# ---- lifecycle --------------------------------------------------------------------------------------------------------------------
def test_lifecycle(ctx):
    import sjhip
    fresh = sjhip.Context(0)
    doc = b'{"o":1,"items":[{"s":"abc","n":1},{"s":"de","n":2.5},{"s":"f","n":-3}]}\n{"o":2,"items":[{"n":null}]}'
    fresh.parse(doc, ndjson=True)
    base = fresh.device_bytes()
    assert fresh.where_path((b"o",), fresh.OP_GE_INT, 2) == (2, 1) and fresh.device_bytes() > base  # the arena of the selection
    assert fresh.fetch_rows(2, 1)[0].tolist() == [0, 0, 1]
    assert fresh.select_rows((b"items",)) == (2, 4)
    assert fresh.where_path((b"n",), fresh.OP_GT_FLOAT, 0.0) == (2, 2)
    off, idx, st = fresh.fetch_rows(2, 2)
    assert off.tolist() == [0, 2, 2] and st.tolist() == [OK, OK]
    nr, nb = fresh.extract_table([((b"s",), S), ((b"n",), F)], fetch=False)
    assert (nr, nb) == (2, [5, 0])
    fresh.select_records()  # a table built under a narrowed selection is materialised data
    with pytest.raises(sjhip.ParseError) as e:
        fresh.fetch_rows(2, 2)
    assert "no row selection" in str(e.value)
    off, data, st = fresh.fetch_table_column(0, nr, S, nb[0])
    assert off.tolist() == [0, 3, 5] and data == b"abcde" and st.tolist() == [OK, OK]
    assert fresh.fetch_table_column(1, nr, F)[0].tolist() == [1.0, 2.5]
    # SJHIP_ERR_ARG leaves the selection bit for bit as it was
    fresh.select_rows((b"items",))
    fresh.where_path((b"n",), fresh.OP_LT_FLOAT, 2.0)
    before = fresh.fetch_rows(2, 2)
    L, h = sjhip.lib(), fresh._h
    import ctypes as C
    lens, nr_, nw_ = (C.c_uint32 * 1)(1), C.c_size_t(77), C.c_size_t(77)
    eight, big = struct.pack("<q", 1), b"x" * 1025
    for op, value, vlen, flags in [(20, eight, 8, 0), (-1, eight, 8, 0), (fresh.OP_GT_INT, eight, 4, 0), (fresh.OP_LE_FLOAT, eight, 0, 0),
                                   (fresh.OP_GE_UINT, None, 8, 0), (fresh.OP_EXISTS, eight, 0, 2), (fresh.OP_EXISTS, eight, 0, 0x80000001),
                                   (fresh.OP_EQ_STRING, big, 1025, 0), (fresh.OP_PREFIX_STRING, big, 1025, 0)]:
        assert L.sjhip_where_path(h, b"n", lens, 1, op, value, vlen, flags, C.byref(nr_), C.byref(nw_)) == 5, (op, vlen, flags)
        for a, b in zip(fresh.fetch_rows(2, 2), before):
            assert np.array_equal(a, b), (op, vlen, flags)
    assert L.sjhip_where_path(h, b"n", lens, 1, 0, None, 0, 0, None, C.byref(nw_)) == 5
    with pytest.raises(sjhip.ParseError):
        fresh.where_path((b"k",) * 17, fresh.OP_EXISTS)
    for a, b in zip(fresh.fetch_rows(2, 2), before):
        assert np.array_equal(a, b)
    # a parse, a failed parse, trim drop it; a call without a result is refused
    for drop in (lambda: fresh.parse(b'{"items":[1]}', ndjson=True), lambda: pytest.raises(sjhip.ParseError, fresh.parse, b'{"s":'),
                 fresh.trim):
        fresh.parse(doc, ndjson=True)
        fresh.where_path((b"o",), fresh.OP_EXISTS)
        drop()
        with pytest.raises(sjhip.ParseError) as e:
            fresh.fetch_rows(2, 2)
        assert "no row selection" in str(e.value)
    assert fresh.device_bytes() == 0  # (after trim: the selection's arena went with the others)
    with pytest.raises(sjhip.ParseError) as e:
        fresh.where_path((b"o",), fresh.OP_EXISTS)
    assert e.value.code == 5
    fresh.close()
    # the narrowed selection survives the other products, the filter, the serializer and MarshalJSON, which ignore it
    doc = wrapped_random(5, 300)
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True, key_flags=True)
    text, stream = ctx.marshal_json(), ctx.serialize()
    n_filtered = ctx.filter_where(b"k", b"HOND")[0]
    sel = RW.select_rows(w, (b"items",))
    ctx.select_rows((b"items",))
    sel = check_where(ctx, w, sel, (b"a",), Q.OP_EXISTS)
    rw = RW.RowWalk(w, sel[1])
    assert ctx.marshal_json() == text and np.array_equal(ctx.serialize(), stream) and ctx.filter_where(b"k", b"HOND")[0] == n_filtered
    assert ctx.count_where(b"k", b"x") == 0
    scol = ctx.extract_path_strings((b"a",), cvt=True)
    lcol = ctx.extract_path_list((b"b",), I)
    tnr, tnb = ctx.extract_table([((b"a",), SC), ((b"b",), I)], fetch=False)
    off, idx, st = ctx.fetch_rows(len(sel[2]), len(sel[1]))
    assert idx.tolist() == sel[1] and off.tolist() == sel[0]
    same_column(S, scol, RW.string_column(rw, (b"a",), True), "column under the narrowed selection")
    assert lcol[0].tolist() == RW.list_column(rw, (b"b",), I)[0]
    same_column(SC, ctx.fetch_table_column(0, tnr, SC, tnb[0]), TW.single(rw, (b"a",), SC), "the table under the narrowed selection")
    ctx.select_records()
    assert ctx.marshal_json() == text


# ---- a sharded result -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ABC", "BAB"])
def test_sharded_result_equals_whole(name):
    import test_gpu_product_parts as PP
    one, many = PP.contexts(name)
    try:
        for op, path, want, negate in [(Q.OP_EXISTS, (b"x",), None, False), (WW.OP_PREFIX_STRING, (b"s",), b"v5", False),
                                       (WW.OP_GE_INT, (b"x",), 100, False), (Q.OP_EXISTS, (b"x",), None, True)]:
            got = []
            for c in (one, many):
                c.select_records()
                nr, rows = c.where_path(path, op, want, negate=negate)
                assert c.count_where_path((b"id",), c.OP_EXISTS) == rows
                sel = c.fetch_rows(nr, rows)
                mid = int(np.median(c.extract_path((b"id",), I)[0]))
                nr2, rows2 = c.where_path((b"id",), WW.OP_GE_INT, mid)  # ... and a second call, which halves every kept stretch
                got.append((nr, rows, sel, nr2, rows2, c.fetch_rows(nr2, rows2), c.extract_table([((b"id",), I), ((b"s",), SC)])))
            a, b = got
            assert a[:2] == b[:2] and a[3:5] == b[3:5] and 0 < a[4] < a[1] < a[0], (name, op, a[:2], a[3:5])
            PP.same(b[2], a[2], (name, op, "rows"))
            PP.same(b[5], a[5], (name, op, "rows, narrowed twice"))
            PP.same(b[6][0], a[6][0], (name, op, "id"))
            PP.same(b[6][1], a[6][1], (name, op, "s"))
    finally:
        one.select_records()
        many.select_records()
