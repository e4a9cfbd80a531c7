"""GPU: the order by several keys (sjhip_order_paths / sjhip_fetch_order) against the serial restatement of
tests/order_multi_walk.py over the oracle's parse: one column against the single-key calls on a second context; two columns on row
counts around the wave and the tile (T rows) with a column 0 that is all equal, all distinct, in pairs across every cut, and in three
classes of which one is a singleton; mixed kinds and directions; the float ties; string keys whose ties end in different rounds, in
both copy modes; every status on either column and on both; eight columns; 70 000 rows; ten limits; under selections, predicates and
an unnest; in front of the consumers of a selection; on twitter and parking; and through the lifecycle and the refusals.

Everything is compared exactly: *records, *rows, the narrowed selection as sjhip_fetch_rows returns it, order and the status bytes
of column 0."""
import ctypes as C
import json
import random

import numpy as np
import pytest

import column_walk as CW
import filter_rows_walk as FW
import fixtures
import marshal_rows_walk as MRW
import order_multi_walk as MW
import query_walk as Q
import rows_walk as RW
import unnest_walk as UW
import where_walk as WW
import workloads
from test_gpu_columns import oracle_walk
from test_gpu_order import T, array_rows, nd_rows, same_selection
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

F, I, U, S = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT, MW.COL_STRING
OK = CW.COL_OK
ERR_ARG = 5
MULTI = -1


def check_order(ctx, w, sel, cols, limit=0, what=None):
    """order_paths on the selection in force (sel: the checker's copy of it, None: no selection) equals the checker.
    -> (what the device returned, the checker's Ordering: its .selection is the selection in force from here on)"""
    what = (what, cols, limit)
    want = MW.order(w, sel, cols, limit)
    got = ctx.order_paths(cols, limit=limit)
    print(what, "records:", got.records, "rows:", got.rows)
    assert (got.records, got.rows, got.kind) == (want.records, want.rows, MULTI) and got.values is None, what
    same_selection(ctx, got.records, got.rows, want.selection, what)
    assert got.order.dtype == np.uint64 and got.order.tolist() == want.order, what
    assert got.status.dtype == np.uint8 and got.status.tolist() == want.status, what
    assert sorted(got.order.tolist()) == list(range(got.rows)), what  # a permutation
    return got, want


def on_records(ctx, w, cols, what, limit=0):
    ctx.select_records()
    out = check_order(ctx, w, None, cols, limit, what)
    ctx.select_records()
    return out


# ---- 1. one column is the single-key call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, T + 1])
def test_one_column_equals_the_single_key_calls(ctx, n):
    import sjhip
    lines = ['{"k":%s}' % ('"s%d"' % (r % 9) if r % 5 == 4 else ("null" if r % 17 == 16 else str((r * 7) % 13 - 3))) for r in range(n)]
    w = nd_rows(ctx, lines)
    other = sjhip.Context(0)
    try:
        other.parse("\n".join(lines).encode(), ndjson=True)
        for kind in (F, I, U, S):
            for desc in (False, True):
                for limit in (0, n // 2 + 1):
                    ctx.select_records(), other.select_records()
                    got, _ = check_order(ctx, w, None, [((b"k",), kind, desc)], limit, ("one column", n))
                    if kind == S:
                        single = other.order_path_strings((b"k",), descending=desc, limit=limit)
                    else:
                        single = other.order_path((b"k",), kind, descending=desc, limit=limit)
                    assert (got.records, got.rows) == (single.records, single.rows)
                    assert np.array_equal(got.order, single.order) and np.array_equal(got.status, single.status)
                    for a, b in zip(ctx.fetch_rows(got.records, got.rows), other.fetch_rows(single.records, single.rows)):
                        assert np.array_equal(a, b)
    finally:
        other.close()
    ctx.select_records()


# ---- 2. row counts and the shapes of column 0 -----------------------------------------------------------------------------------------------
FIRST = {
    "all-equal": lambda r, n: 7,  # everything reaches column 1
    "all-distinct": lambda r, n: (r * 7919) % 100003,  # nothing does
    "pairs": lambda r, n: (r + 1) // 2,  # rows 2 j - 1 and 2 j: a pair straddles every even cut -- 64, T, 2 T
    "three-classes": lambda r, n: 1 if r == n // 2 else (0 if r % 2 else 2),  # one of them a singleton
}


@pytest.mark.parametrize("pattern", sorted(FIRST))
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_row_counts(ctx, n, pattern):
    w = nd_rows(ctx, ['{"a":%d,"b":%d}' % (FIRST[pattern](r, n), (r * 31) % 17) for r in range(n)])
    got, _ = on_records(ctx, w, [((b"a",), I, False), ((b"b",), U, True)], (pattern, n))
    if pattern == "all-equal":  # column 1 alone, descending, stable
        assert got.order.tolist() == sorted(range(n), key=lambda r: -((r * 31) % 17))
    if pattern == "pairs" and n > 2:
        assert got.order.tolist()[:3] == [0] + ([1, 2] if 31 % 17 > 62 % 17 else [2, 1])
    on_records(ctx, w, [((b"a",), F, True), ((b"b",), I, False)], (pattern, n, "descending"))


# ---- 3. kinds ---------------------------------------------------------------------------------------------------------------------------
def mixed_lines(n):
    rnd = random.Random(n)
    names = ["VW", "BMW", "AUDI", "MERCEDES-BENZ", "MERCEDES", "", "Škoda", "VOLKSWAGEN AG 1", "VOLKSWAGEN AG 2"]
    return ['{"s":%s,"i":%d,"f":%s,"u":%d}' % (json.dumps(rnd.choice(names)), rnd.randrange(-3, 4), rnd.choice(("1.5", "-2", "0", "1e3", "1.50")),
                                               rnd.randrange(5)) for _ in range(n)]


@pytest.mark.parametrize("cols", [[((b"s",), S, False), ((b"i",), I, False)], [((b"i",), I, True), ((b"s",), S, True)],
                                  [((b"f",), F, True), ((b"s",), S, False), ((b"u",), U, True)]], ids=["string-int", "int-string", "float-string-uint"])
def test_mixed_kinds(ctx, cols):
    w = nd_rows(ctx, mixed_lines(T + 1))
    on_records(ctx, w, cols, "mixed")


def test_float_ties(ctx):
    # 0.0 and the integer 0 tie under FLOAT and meet column 1; -0.0 lies below both
    rows = ['{"f":0.0,"t":"c"}', '{"f":-0.0,"t":"z"}', '{"f":0,"t":"a"}', '{"f":0.0,"t":"b"}', '{"f":-0.0,"t":"y"}', '{"f":1,"t":"a"}', '{"f":0,"t":"c"}',
            '{"f":-1e-300,"t":"a"}']
    w, sel = array_rows(ctx, rows)
    got, _ = check_order(ctx, w, sel, [((b"f",), F, False), ((b"t",), S, False)], 0, "float ties")
    assert got.order.tolist() == [7, 4, 1, 2, 3, 0, 6, 5]
    ctx.select_rows((b"rows",))
    got, _ = check_order(ctx, w, sel, [((b"f",), F, True), ((b"t",), S, True)], 0, "float ties, descending")
    assert got.order.tolist() == [5, 0, 6, 3, 2, 1, 4, 7]
    ctx.select_records()


@pytest.mark.parametrize("copy", [True, False], ids=["copied", "in-the-message"])
def test_string_ties_that_end_in_different_rounds(ctx, copy):
    # column-0 keys of 0, 6, 7, 8, 13, 14, 15 and 21 bytes, three of each: their ties end in rounds 1 .. 4 and meet again in column 1
    stem = "abcdefghijklmnopqrstu"
    rnd = random.Random(4)
    rows = []
    for length in (0, 6, 7, 8, 13, 14, 15, 21):
        for j in range(3):
            text = stem[:length]
            if j == 1 and length:  # an escaped spelling of the same key
                text = "\\u0061" + text[1:]
            rows.append('{"k":"%s","v":%d}' % (text, rnd.randrange(2)))
    rows += ['{"k":"abcdefX","v":1}', '{"k":"abcdefghijklmX","v":0}', '{"v":3}']
    rnd.shuffle(rows)
    w, sel = array_rows(ctx, rows, copy=copy)
    for desc in (False, True):
        ctx.select_rows((b"rows",))
        got, _ = check_order(ctx, w, sel, [((b"k",), S, desc), ((b"v",), I, not desc)], 0, "different rounds")
        assert got.status.tolist() == [OK] * 26 + [CW.COL_NOT_FOUND]
    ctx.select_records()


# ---- 4. statuses --------------------------------------------------------------------------------------------------------------------------
STATUS_ROWS = ['{"a":1,"b":"x"}', '{"a":1}', '{"b":"a"}', '{"a":1,"b":"c"}', '{"a":0,"b":null}', '{"a":0,"b":"z"}', '{"b":7}', '7', '{"a":"s","b":"a"}',
               '{"a":null,"b":"a"}', '{"a":-1,"b":[1]}', '{"a":18446744073709551615,"b":"q"}', '{"a":1.5,"b":"q"}', '{"a":1e30,"b":"p"}', '"s"',
               '{"a":{"a":1},"b":{"b":"x"}}', '{"a":1,"b":true}', '{"a":null}', '{"a":null,"b":null}']


def test_every_status_on_either_column_and_on_both(ctx):
    w, sel = array_rows(ctx, STATUS_ROWS)
    seen = set()
    for cols in ([((b"a",), I, False), ((b"b",), S, False)], [((b"a",), U, True), ((b"b",), S, True)], [((b"b",), S, False), ((b"a",), I, True)],
                 [((b"a",), F, False), ((b"b",), I, False)], [((b"nope",), I, False), ((b"a", b"a"), U, False), ((b"b",), S, True)]):
        ctx.select_rows((b"rows",))
        got, want = check_order(ctx, w, sel, cols, 0, "statuses")
        seen |= set(want.status)
    assert seen == {OK, CW.COL_NOT_FOUND, CW.COL_NOT_OBJECT, CW.COL_NULL, CW.COL_TYPE, CW.COL_RANGE}
    # the rows without a key on column 0 are ordered among themselves by column 1; without one on every column: row order
    ctx.select_rows((b"rows",))
    got, _ = check_order(ctx, w, sel, [((b"nope",), I, False), ((b"b",), S, False)], 0, "missing everywhere on column 0")
    assert set(got.status.tolist()) == {CW.COL_NOT_FOUND, CW.COL_NOT_OBJECT} and got.order.tolist()[:3] == [2, 8, 9]
    ctx.select_rows((b"rows",))
    got, _ = check_order(ctx, w, sel, [((b"nope",), I, False), ((b"no", b"no"), S, True)], 0, "missing everywhere")
    assert got.order.tolist() == list(range(len(STATUS_ROWS)))
    ctx.select_records()


def test_every_status_on_column_1_only(ctx):
    # column 0 is OK everywhere and ties in two classes; column 1's path (b, x) is OK, NOT_FOUND (no b, no x), NOT_OBJECT (b is a
    # scalar), NULL, TYPE and RANGE: within each class the rows without a key come last, in row order
    rows = ['{"a":1,"b":{"x":5}}', '{"a":1,"b":5}', '{"a":1}', '{"a":1,"b":{"x":null}}', '{"a":1,"b":{"x":2}}', '{"a":0,"b":"s"}', '{"a":0,"b":{"x":"t"}}',
            '{"a":0,"b":{"x":7}}', '{"a":0,"b":{"y":1}}', '{"a":1,"b":{"x":-1}}', '{"a":0,"b":{"x":1e30}}', '{"a":0,"b":[1]}', '{"a":0,"b":{"x":7}}']
    w, sel = array_rows(ctx, rows)
    column_1 = MW.columns(w, [int(i) for i in sel[1]], [((b"b", b"x"), U, False)])[0][3]
    assert set(column_1) == {OK, CW.COL_NOT_FOUND, CW.COL_NOT_OBJECT, CW.COL_NULL, CW.COL_TYPE, CW.COL_RANGE}
    assert column_1[1] == column_1[5] == column_1[11] == CW.COL_NOT_OBJECT
    got, _ = check_order(ctx, w, sel, [((b"a",), I, False), ((b"b", b"x"), U, False)], 0, "statuses on column 1 only")
    assert got.order.tolist() == [7, 12, 5, 6, 8, 10, 11, 4, 0, 1, 2, 3, 9] and got.status.tolist() == [OK] * 13
    ctx.select_rows((b"rows",))
    got, _ = check_order(ctx, w, sel, [((b"a",), I, True), ((b"b", b"x"), U, True)], 0, "statuses on column 1 only, descending")
    assert got.order.tolist() == [0, 4, 1, 2, 3, 9, 7, 12, 5, 6, 8, 10, 11]
    ctx.select_records()


def test_empty_paths_the_rows_own_values(ctx):
    # path_lens[c] == 0: the key is the row's own value -- alone, in front of a column with a path, behind one, and twice
    doc = b'{"n":["pear",3,"apple","",null,"pear",["x"],"fig",3,2.5,"apple",-1,{"k":1},3]}'
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = RW.select_rows(w, (b"n",))
    for cols, head in (([((), S, False), ((), F, True)], [3, 2, 10, 7, 0, 5, 1, 8, 13, 9, 11]),
                       ([((), F, True), ((), S, False)], [1, 8, 13, 9, 11, 3, 2, 10, 7, 0, 5]),
                       ([((), I, False)], None), ([((b"k",), U, False), ((), S, True)], [12, 0, 5, 7, 2, 10, 3]),
                       ([((), S, True), ((b"k",), U, False)], None)):
        ctx.select_rows((b"n",))
        got, _ = check_order(ctx, w, sel, cols, 0, "own values")
        assert got.rows == 14 and (head is None or got.order.tolist()[:len(head)] == head), got.order.tolist()
    ctx.select_rows((b"n",))
    got, want = check_order(ctx, w, sel, [((), S, True), ((), I, False)], 4, "own values, the first 4")
    assert got.order.tolist() == [0, 2, 3, 1] and want.selection[1] == [sel[1][r] for r in (0, 2, 5, 7)]  # pear, pear, fig, apple
    ctx.select_records()


def test_eight_columns(ctx):
    n = 2 * T + 3  # column c halves the classes of column c - 1; the eighth decides inside what the seven left tied
    w = nd_rows(ctx, ['{%s,"h":%d}' % (",".join('"c%d":%d' % (c, (r >> (10 - c)) & 1) for c in range(7)), r % 3) for r in range(n)])
    cols = [((b"c%d" % c,), (I, U, F)[c % 3], c % 2 == 1) for c in range(7)] + [((b"h",), I, True)]
    on_records(ctx, w, cols, "eight columns")
    on_records(ctx, w, cols, "eight columns, limit", 100)


def test_seventy_thousand_rows(ctx):
    """70 000 rows, about 300 distinct strings on column 0 and a random int64 on column 1: 69 tiles in every scan and histogram."""
    rnd = random.Random(70)
    n = 70000
    names = ["make %03d" % d if d % 3 else "a longer make name %03d" % d for d in range(300)]
    w = nd_rows(ctx, ['{"m":%s,"v":%d}' % ("null" if r % 997 == 0 else '"%s"' % rnd.choice(names), rnd.randrange(-1 << 63, 1 << 63)) for r in range(n)])
    got, _ = check_order(ctx, w, None, [((b"m",), S, False), ((b"v",), I, True)], 0, "70000")
    assert got.rows == n
    ctx.select_records()
    got, _ = check_order(ctx, w, None, [((b"m",), S, True), ((b"v",), I, False)], 1000, "70000, the first 1000")
    assert got.rows == 1000
    ctx.select_records()


# ---- 5. limits ----------------------------------------------------------------------------------------------------------------------------
N_LIMIT = 2 * T + 3


def limit_lines():
    # column 0 has 6 values; column 1 has 40 inside each, so every class of (a, b) holds about 8 rows that only the row order separates
    return ['{"a":%d,"b":%s}' % (r % 6, "null" if r % 11 == 10 else str((r * 7) % 40)) for r in range(N_LIMIT)]


@pytest.mark.parametrize("limit", [1, 2, 340, 343, T, T + 1, N_LIMIT - 1, N_LIMIT, N_LIMIT + 5, 0])
def test_limits(ctx, limit):
    w = nd_rows(ctx, limit_lines())
    got, want = on_records(ctx, w, [((b"a",), U, False), ((b"b",), I, True)], "limit", limit)
    assert got.rows == (N_LIMIT if limit == 0 or limit >= N_LIMIT else limit)


def test_limits_that_cut_a_class(ctx):
    rows = ['{"a":1,"b":3}', '{"a":1,"b":1}', '{"a":1,"b":2}', '{"a":0,"b":9}', '{"a":1,"b":1}']
    w, sel = array_rows(ctx, rows)
    got, want = check_order(ctx, w, sel, [((b"a",), U, False), ((b"b",), U, False)], 2, "only the row order separates")
    assert got.order.tolist() == [1, 0] and want.selection[1] == [sel[1][1], sel[1][3]]
    ctx.select_rows((b"rows",))
    got, want = check_order(ctx, w, sel, [((b"a",), U, False), ((b"b",), U, False)], 4, "only column 1 separates")
    assert got.order.tolist() == [2, 0, 3, 1]
    ctx.select_records()


# ---- 6. composition -----------------------------------------------------------------------------------------------------------------------
ITEM_LINES = ['{"items":[{"id":1,"v":"d","n":2},{"id":2,"v":"k","n":1},{"id":3,"v":"d","n":1}]}', '{"items":[]}', '{"x":1}', '{"items":[{"id":4,"v":"h","n":0}]}',
              '{"items":7}', '{"items":[{"id":5,"v":"i","n":5},{"id":6,"v":"d"},{"id":7},{"id":8,"v":"i","n":4},{"id":9,"v":"","n":1}]}',
              '{"items":[{"id":10,"v":"d","n":2}]}']


@pytest.mark.parametrize("limit", [0, 1, 4, 10])
def test_records_that_own_no_one_and_many_rows(ctx, limit):
    doc = "\n".join(ITEM_LINES).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    sel = RW.select_rows(w, (b"items",))
    assert ctx.select_rows((b"items",)) == (7, 10)
    got, want = check_order(ctx, w, sel, [((b"v",), S, False), ((b"n",), I, True)], limit, "items")
    assert want.selection[2] == sel[2] and got.records == 7
    check_order(ctx, w, want.selection, [((b"n",), U, False), ((b"id",), I, True)], 3, "items, again")  # on what the first left
    ctx.select_records()


@pytest.mark.parametrize("copy", [True, False], ids=["copied", "in-the-message"])
def test_with_a_row_predicate_in_front_and_behind(ctx, copy):
    rows = ['{"id":%d,"v":"name %03d","t":"%s","g":%d}' % (r, (r * 37) % 101, "ab"[r % 2], r % 5) for r in range(300)]
    w, sel = array_rows(ctx, rows, copy=copy)
    narrowed = WW.where(w, sel, (b"t",), Q.OP_EQ_STRING, b"a")
    assert ctx.where_path((b"t",), ctx.OP_EQ_STRING, b"a") == (1, 150)
    got, want = check_order(ctx, w, narrowed, [((b"g",), I, True), ((b"v",), S, False)], 40, "where, then order")
    after = WW.where(w, want.selection, (b"id",), WW.OP_GE_INT, 150)
    assert ctx.where_path((b"id",), ctx.OP_GE_INT, 150) == (1, len(after[1]))
    same_selection(ctx, 1, len(after[1]), after, "order, then where")
    check_order(ctx, w, after, [((b"g",), U, False), ((b"v",), S, True)], 2, "and order again")
    ctx.select_records()


def test_behind_an_unnest_on_twitter_hashtags(ctx):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = RW.select_rows(w, (b"statuses",))
    assert ctx.select_rows((b"statuses",)) == (1, len(sel[1]))
    offs, index, sts = UW.unnest_rows(RW.RowWalk(w, sel[1]), (b"entities", b"hashtags"), sel[0], sel[2])[:3]
    assert ctx.unnest_rows((b"entities", b"hashtags"))[2] == len(index) >= 2
    check_order(ctx, w, (offs, index, sts), [((b"text",), S, False), ((b"indices",), I, False)], 0, "hashtags")
    ctx.select_records()


TEXT_ROWS = ['{"id":%d,"v":"%s","n":%d}' % (r, "key %02d" % ((r * 61) % 97), r % 7) for r in range(200)]


@pytest.mark.parametrize("copy", [True, False], ids=["copied", "in-the-message"])
def test_the_consumers_of_the_selection_see_the_kept_rows(ctx, copy):
    k = 10
    w, sel = array_rows(ctx, TEXT_ROWS, copy=copy)
    got, want = check_order(ctx, w, sel, [((b"n",), I, True), ((b"v",), S, False)], k, "top k")
    by_key = sorted(range(200), key=lambda r: (-(r % 7), (r * 61) % 97, r))[:k]
    n, text, off = ctx.marshal_rows(offsets=True)
    lines = [text[int(off[i]):int(off[i + 1]) - 1] for i in range(n)]
    assert n == k and [lines[i] for i in got.order.tolist()] == [TEXT_ROWS[r].encode() for r in by_key]
    want_text, want_off = MRW.marshal_rows(w, want.selection[1])
    assert text == want_text and off.tolist() == [int(x) for x in want_off]
    (ids, st), (soff, sdata, sst) = ctx.extract_table([((b"id",), I), ((b"v",), ctx.COL_STRING)])  # the sorted keys: the table through order
    assert ids[got.order.astype(np.int64)].tolist() == by_key and st.tolist() == [0] * k
    names = [sdata[int(a):int(b)] for a, b in zip(soff[:-1], soff[1:])]
    assert [names[i] for i in got.order.tolist()] == [b"key %02d" % ((r * 61) % 97) for r in by_key]
    agg = ctx.aggregate_path((b"id",), I)
    assert (agg.rows, agg.max, agg.min) == (k, max(by_key), min(by_key))
    if copy:
        tape, strings, skipped = FW.filter_rows(w, want.selection[1])
        n_rows, skipped_got, pj = ctx.filter_rows()
        assert (n_rows, skipped_got) == (k, skipped) and pj.Tape.tolist() == tape and pj.Strings.tobytes() == strings
    ctx.select_records()


def test_twitter(ctx):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = RW.select_rows(w, (b"statuses",))
    assert ctx.select_rows((b"statuses",)) == (1, len(sel[1]))
    got, want = check_order(ctx, w, sel, [((b"user", b"screen_name"), S, False), ((b"retweet_count",), I, True)], 0, "screen names, most retweeted first")
    assert set(want.status) == {OK} and got.rows == len(sel[1])
    got, want = check_order(ctx, w, sel, [((b"user", b"lang"), S, False), ((b"retweet_count",), I, True), ((b"id",), U, False)], 5, "five")
    n, text = ctx.marshal_rows()
    assert n == 5 and text == MRW.marshal_rows(w, want.selection[1])[0]
    ctx.select_records()


def test_parking_by_make_and_color(ctx):
    doc = b"\n".join(workloads.c5_parking_nd(3).split(b"\n")[:3000])
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    on_records(ctx, w, [((b"Make",), S, False), ((b"Color",), S, False)], "parking")
    on_records(ctx, w, [((b"Make",), S, True), ((b"Color",), S, False), ((b"Fine",), F, True)], "parking, three keys", 10)


# ---- 7. lifecycle, refusals -----------------------------------------------------------------------------------------------------------------
def same_order(a, b):
    assert (a.records, a.rows, a.kind) == (b.records, b.rows, b.kind)
    assert np.array_equal(a.order, b.order) and np.array_equal(a.status, b.status)
    assert (a.values is None and b.values is None) or np.array_equal(a.values, b.values)


TWO = [((b"user", b"screen_name"), S, False), ((b"retweet_count",), I, True)]


def test_lifecycle(ctx):
    import sjhip
    L = sjhip.lib()
    doc = fixtures.load("twitter")
    ctx.trim()
    ctx.parse(doc, key_flags=True)
    ctx.select_rows((b"statuses",))
    before = ctx.device_bytes()
    first = ctx.order_paths(TWO, limit=30)
    assert ctx.device_bytes() > before and first.kind == MULTI and first.values is None
    ctx.select_rows((b"statuses",))
    same_order(ctx.order_paths(TWO, limit=30), first)  # the same bits again
    # a non-NULL values: an argument error that says where the keys come from, and the order stays
    buf = np.zeros(30, dtype=np.uint64)
    assert L.sjhip_fetch_order(ctx._h, None, buf.ctypes.data, None) == ERR_ARG
    assert "no 8-byte values" in ctx.last_error() and "sjhip_extract_table" in ctx.last_error()
    same_order(ctx.fetch_order(sjhip.Order(1, 30, MULTI)), first)
    # a single-key order replaces it, and it replaces that
    ctx.select_rows((b"statuses",))
    numeric = ctx.order_path((b"retweet_count",), I, descending=True, limit=7)
    assert numeric.kind == I and L.sjhip_fetch_order(ctx._h, None, buf.ctypes.data, None) == 0
    ctx.select_rows((b"statuses",))
    assert ctx.order_path_strings((b"lang",), limit=9).rows == 9
    ctx.select_rows((b"statuses",))
    same_order(ctx.order_paths(TWO, limit=30), first)
    # it survives the drop and the change of the selection and every other product ...
    ctx.select_records()
    ctx.select_rows((b"statuses",))
    ctx.extract_path_strings((b"lang",))
    ctx.extract_path_list((b"entities", b"hashtags"), I)
    ctx.extract_table([((b"retweet_count",), I), ((b"lang",), ctx.COL_STRING)])
    ctx.group_path((b"lang",), ctx.COL_STRING, (b"retweet_count",), I)
    ctx.where_path((b"lang",), ctx.OP_EQ_STRING, b"ja")
    ctx.filter_rows(fetch=False)
    ctx.serialize(fetch=False)
    ctx.marshal_rows(fetch=False)
    text = ctx.marshal_json()
    same_order(ctx.fetch_order(sjhip.Order(1, 30, MULTI)), first)
    # ... and they survive it
    ctx.select_rows((b"statuses",))
    groups = ctx.group_path((b"lang",), ctx.COL_STRING, (b"retweet_count",), I, fetch=False)
    column = ctx.extract_path_strings((b"lang",), fetch=False)
    ctx.order_paths([((b"lang",), S, True), ((b"id",), U, False)], limit=7)
    kept = ctx.fetch_rows(1, 7)
    g = ctx.fetch_groups(groups)
    assert sorted(g.keys) == [b"ja", b"zh"] and len(ctx.fetch_path_strings(*column)[1]) == 200
    assert ctx.marshal_rows(fetch=False)[0] == 7 and ctx.marshal_json() == text
    # the refusals touch nothing: the selection and the order are bit for bit as before
    previous = ctx.fetch_order(sjhip.Order(1, 7, MULTI))
    nr, nw = C.c_size_t(77), C.c_size_t(77)
    out = (C.byref(nr), C.byref(nw))
    key_lens = (C.c_uint32 * 9)(*([4] * 9))
    path_lens = (C.c_uint32 * 9)(*([1] * 9))
    kinds = (C.c_int * 9)(*([1] * 9))
    flags = (C.c_uint32 * 9)(*([0] * 9))
    keys = b"lang" * 9
    call = lambda n_cols, *tail: L.sjhip_order_paths(ctx._h, keys, key_lens, path_lens, kinds, flags, n_cols, 3, *(tail or out))  # noqa: E731
    for n_cols in (0, 9):
        assert call(n_cols) == ERR_ARG and "%d key columns" % n_cols in ctx.last_error()
    for bad in (3, 5, 17, -1):  # SJHIP_COL_BOOL, SJHIP_COL_STRING_CVT, unknown
        kinds[1] = bad
        assert call(2) == ERR_ARG and "column 1" in ctx.last_error() and "kind %d" % bad in ctx.last_error(), ctx.last_error()
    kinds[1] = 4
    for bits, word in [(2, "flag bits 0x2"), (0x80000001, "flag bits 0x80000000")]:
        flags[2] = bits
        assert call(3) == ERR_ARG and "column 2" in ctx.last_error() and word in ctx.last_error(), ctx.last_error()
    flags[2] = 0
    assert call(2, None, None) == ERR_ARG and "null" in ctx.last_error()
    with pytest.raises(sjhip.ParseError):
        ctx.order_paths([((b"k",) * 17, I, False)])  # a path longer than sjhip_find_path takes
    with pytest.raises(sjhip.ParseError):
        ctx.order_paths([((b"k",) * 9, I, False)] * 4)  # 36 keys over all paths
    assert (nr.value, nw.value) == (77, 77)
    same_order(ctx.fetch_order(sjhip.Order(1, 7, MULTI)), previous)
    for a, b in zip(ctx.fetch_rows(1, 7), kept):
        assert np.array_equal(a, b)
    assert call(2) == 0 and (nr.value, nw.value) == (1, 3)  # (and the same arguments, mended, are taken)
    # a selection without rows: nothing is launched, an empty order is published and fetched
    assert ctx.where_path((b"lang",), ctx.OP_EQ_STRING, b"en") == (1, 0)
    empty = ctx.order_paths(TWO, limit=3)
    assert (empty.records, empty.rows, len(empty.order), empty.values, len(empty.status)) == (1, 0, 0, None, 0)
    assert ctx.fetch_rows(1, 0)[0].tolist() == [0, 0]
    ctx.select_records()
    # a parse drops it; so does a trim, which frees its arena
    ctx.parse(b'{"a":"x","b":1}')
    assert L.sjhip_fetch_order(ctx._h, None, None, None) == ERR_ARG and "no order" in ctx.last_error()
    one = ctx.order_paths([((b"a",), S, False), ((b"b",), I, False)])
    assert (one.records, one.rows, one.order.tolist(), one.status.tolist()) == (1, 1, [0], [0])
    ctx.trim()
    assert ctx.device_bytes() == 0 and L.sjhip_fetch_order(ctx._h, None, None, None) == ERR_ARG
    fresh = sjhip.Context(0)  # no result on the device
    assert L.sjhip_order_paths(fresh._h, keys, key_lens, path_lens, kinds, flags, 2, 0, *out) == ERR_ARG and fresh.last_error()
    fresh.close()


def test_sharded_result_is_refused(ctx):
    import sjhip
    pad = "x" * 230
    doc = "\n".join('{"pad":"%s","k":"%d","v":%d}' % (pad, r % 7, r) for r in range(11000)).encode()
    assert len(doc) > 5 << 19
    many = sjhip.Context(0)
    try:
        with fixtures.nd_shard_limits(2 << 20, 1 << 20):
            many.parse(doc, ndjson=True)
        with pytest.raises(sjhip.ParseError):
            many.order_paths([((b"k",), S, False), ((b"v",), I, True)])
        assert "is sharded" in many.last_error()
        assert many.aggregate_path((b"k",), I).status[CW.COL_TYPE] == 11000  # the result is as it was
    finally:
        many.close()
