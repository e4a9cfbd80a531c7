"""GPU: the string order (sjhip_order_path_strings / sjhip_fetch_order) against the serial restatement of
tests/order_strings_walk.py over the oracle's parse: on row counts around the wave and the sort tile (T rows) with equal, distinct,
alternating, ascending and descending keys in both directions; on key lengths around the 7-byte chunk of a round, on keys that end
exactly at a chunk, that differ only in their last byte after 0, 1, 2 and 28 whole chunks, on prefix chains, NUL bytes and bytes
above 0x7F; on several classes refined in one round; on escaped spellings in both copy modes; on every status; on limits; on 70 000
rows; under selections, predicates and an unnest; in front of the consumers of a selection; on twitter and parking; and through the
lifecycle and the error paths.

Everything is compared exactly: *records, *rows, the narrowed selection as sjhip_fetch_rows returns it, order, the status bytes, and
the sorted keys -- sjhip_extract_path_strings on the kept rows, taken through order."""
import ctypes as C
import json
import random

import numpy as np
import pytest

import column_walk as CW
import filter_rows_walk as FW
import fixtures
import marshal_rows_walk as MW
import order_strings_walk as SW
import order_walk as OW
import query_walk as Q
import rows_walk as RW
import unnest_walk as UW
import where_walk as WW
import workloads
from test_group_walk import STATUS_DOC
from test_gpu_columns import oracle_walk
from test_gpu_order import LACKING, N_LIMIT, N_OK, T, array_rows, lacking_cut, nd_rows, same_selection
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

I, F = CW.COL_INT, CW.COL_FLOAT
S = SW.COL_STRING
ERR_ARG = 5
OK = CW.COL_OK


def js(key):
    """the JSON text of a key given as bytes (UTF-8) or str"""
    return json.dumps(key.decode() if isinstance(key, bytes) else key, ensure_ascii=False)


def column_keys(ctx, path):
    off, data, st = ctx.extract_path_strings(path)
    return [data[int(a):int(b)] for a, b in zip(off[:-1], off[1:])], st.tolist()


def check_order(ctx, w, sel, path, descending=False, limit=0, what=None):
    """order_path_strings on the selection in force (sel: the checker's copy of it, None: no selection) equals the checker.
    -> (what the device returned, the checker's Ordering: its .selection is the selection in force from here on)"""
    what = (what, path, descending, limit)
    want = SW.order(w, sel, path, descending, limit)
    got = ctx.order_path_strings(path, descending=descending, limit=limit)
    longest = max([len(k) for k in want.values if k is not None] or [0])
    print(what, "records:", got.records, "rows:", got.rows, "longest key:", longest, "rounds at most:", SW.max_rounds(longest))
    assert (got.records, got.rows, got.kind) == (want.records, want.rows, S) and got.values is None, what
    same_selection(ctx, got.records, got.rows, want.selection, what)
    assert got.order.dtype == np.uint64 and got.order.tolist() == want.order, what
    assert got.status.dtype == np.uint8 and got.status.tolist() == want.status, what
    assert sorted(got.order.tolist()) == list(range(got.rows)), what  # a permutation
    if len(path) and got.rows:  # the sorted keys: the string column of the kept rows, taken through order
        keys, sts = column_keys(ctx, path)
        assert [keys[i] for i in got.order.tolist()] == [k or b"" for k in want.values], what
        assert [sts[i] for i in got.order.tolist()] == want.status, what
    return got, want


def both_directions(ctx, w, path, what, limit=0):
    """on the records of an ND document: ascending and descending, each from no selection"""
    out = []
    for desc in (False, True):
        ctx.select_records()
        out.append(check_order(ctx, w, None, path, desc, limit, what))
    ctx.select_records()
    return out


def key_rows(ctx, keys):
    return nd_rows(ctx, ['{"k":%s}' % js(k) for k in keys])


# ---- 1. shapes: the wave, the tile, five key patterns, two directions ---------------------------------------------------------------------
PATTERNS = {
    "all-equal": lambda r, n: "same key",
    "all-distinct": lambda r, n: "k%05d" % ((r * 7919) % 100003),
    "two-alternating": lambda r, n: ("pear", "apple")[r % 2],
    "ascending": lambda r, n: "row %06d" % r,
    "descending": lambda r, n: "row %06d" % (n - r),
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_shapes(ctx, n, pattern):
    w = key_rows(ctx, [PATTERNS[pattern](r, n) for r in range(n)])
    (asc, _), (desc, _) = both_directions(ctx, w, (b"k",), (pattern, n))
    if pattern in ("all-equal", "ascending"):
        assert asc.order.tolist() == list(range(n))
    if pattern == "all-equal":
        assert desc.order.tolist() == list(range(n))
    if pattern == "two-alternating" and n > 1:  # stability across waves, rounds and tiles: each key's rows in row order
        assert asc.order.tolist() == list(range(1, n, 2)) + list(range(0, n, 2))
        assert desc.order.tolist() == list(range(0, n, 2)) + list(range(1, n, 2))


# ---- 1b. rows without a key at the seams: they travel through the sort as the missing bit of the class key ------------------------------
SEAM_KEYS = ("", "abcdefg", "abcdefgh", "abcdefg", "", "abcdefgi")  # 0, 7 and 8 bytes: classes that end in round 0 and in round 1


@pytest.mark.parametrize("pattern", sorted(LACKING))
@pytest.mark.parametrize("n", [1, 2, 64, 65, OW.QTILE, OW.QTILE + 1])
def test_rows_without_a_key_at_the_seams(ctx, n, pattern):
    has = [LACKING[pattern](r, n) for r in range(n)]
    # (the keys repeat, so rows tie; a row without one lacks the member, or holds a null or a number)
    w = nd_rows(ctx, ['{"k":%s}' % js(SEAM_KEYS[(r * 5) % 6]) if has[r] else ('{"x":%d}' % r, '{"k":null}', '{"k":7}')[r % 3] for r in range(n)])
    for limit in (0, lacking_cut(has)):
        for got, want in both_directions(ctx, w, (b"k",), (pattern, n), limit):
            kept = n if limit == 0 else min(n, limit)
            tail = kept - min(kept, has.count(True))  # the kept rows without a key: behind the others, in row order
            assert got.rows == kept and [st != OK for st in got.status.tolist()] == [False] * (kept - tail) + [True] * tail
            assert got.order.tolist()[kept - tail:] == sorted(got.order.tolist()[kept - tail:])


# ---- 2. the rounds ----------------------------------------------------------------------------------------------------------------------
def test_key_lengths_around_the_chunk(ctx):
    rnd = random.Random(7)
    keys = []
    for length in (0, 1, 6, 7, 8, 13, 14, 15, 21):
        for _ in range(12):  # a shared stem, so that keys of different lengths tie for whole chunks
            keys.append(("abcdefghijklmnopqrstu"[:length - 1] + rnd.choice("ux")) if length else "")
        keys.append("abcdefghijklmnopqrstu"[:length])
    rnd.shuffle(keys)
    w = key_rows(ctx, keys)
    both_directions(ctx, w, (b"k",), "lengths")


def test_equal_keys_that_end_with_a_full_chunk(ctx):
    # exactly 7 and exactly 14 bytes: only the round BEHIND the full chunk sees the end (a chunk of count 0)
    keys = ["abcdefg", "abcdefgabcdefg", "abcdefg", "abcdef", "abcdefgabcdefg", "abcdefg", "abcdefgabcdefgh", "abcdefgabcdefg"]
    w = key_rows(ctx, keys * 5)
    (asc, want), _ = both_directions(ctx, w, (b"k",), "round end")
    assert [k for k in want.values[:6]] == [b"abcdef"] * 5 + [b"abcdefg"]
    w = key_rows(ctx, ["abcdefg"] * (T + 1))
    (asc, _), (desc, _) = both_directions(ctx, w, (b"k",), "one class of 7 bytes")
    assert asc.order.tolist() == list(range(T + 1)) == desc.order.tolist()


@pytest.mark.parametrize("stem", [0, 7, 14, 199], ids=lambda s: "stem-%d" % s)
def test_keys_that_differ_in_their_last_byte_only(ctx, stem):
    # equal through stem / 7 whole chunks; 199 + 1 bytes: 29 rounds
    rnd = random.Random(stem)
    keys = ["s" * stem + chr(0x30 + rnd.randrange(40)) for _ in range(150)]
    w = key_rows(ctx, keys)
    (asc, want), _ = both_directions(ctx, w, (b"k",), ("late difference", stem))
    assert want.values == sorted(k.encode() for k in keys) and SW.refine([k.encode() for k in keys])[1] == stem // 7 + 1


def test_prefix_chain(ctx):
    chain = ["abcdefghijklmno"[:k] for k in range(16)]
    keys = chain * 3
    random.Random(3).shuffle(keys)
    w = key_rows(ctx, keys)
    (asc, want), (desc, dwant) = both_directions(ctx, w, (b"k",), "prefix chain")
    assert want.values[::3] == [k.encode() for k in chain] and dwant.values[::3] == [k.encode() for k in chain[::-1]]


@pytest.mark.parametrize("copy", [True, False], ids=["copied", "in-the-message"])
def test_nul_non_ascii_and_escaped_spellings(ctx, copy):
    rows = ['{"k":"a\\u0000\\u0000"}', '{"k":"a\\u0000"}', '{"k":"a"}', '{"k":"z"}', '{"k":"é"}', '{"k":"\U0001F600"}', '{"k":"A"}', '{"k":"\\u0041"}',
            '{"k":"\\u00e9"}', '{"k":""}', '{"k":"a\\u0000b"}', '{"k":"\\u0061"}', '{"k":"abcdefg\\u0000"}', '{"k":"abcdefg"}', '{"k":"abcdef\\u0067"}']
    w, sel = array_rows(ctx, rows, copy=copy)
    got, want = check_order(ctx, w, sel, (b"k",), False, 0, "bytes")
    assert want.values == [b"", b"A", b"A", b"a", b"a", b"a\0", b"a\0\0", b"a\0b", b"abcdefg", b"abcdefg", b"abcdefg\0", b"z", b"\xc3\xa9", b"\xc3\xa9",
                           b"\xf0\x9f\x98\x80"]
    assert got.order.tolist() == [9, 6, 7, 2, 11, 1, 0, 10, 13, 14, 12, 3, 4, 8, 5]
    ctx.select_rows((b"rows",))
    got, _ = check_order(ctx, w, sel, (b"k",), True, 0, "bytes, descending")
    assert got.order.tolist() == [5, 4, 8, 3, 12, 13, 14, 10, 0, 1, 2, 11, 6, 7, 9]
    ctx.select_records()


def test_several_classes_refined_in_one_round(ctx):
    # T + 1 rows over 300 distinct 10-byte keys that share their first 7 bytes in groups: round 1 sorts many classes at once
    rnd = random.Random(11)
    distinct = ["%s%03d" % (("grpAAAA", "grpBBBB", "grpCCCC", "grpéé")[d % 4], d) for d in range(300)]
    assert all(len(k.encode()) == 10 for k in distinct)
    keys = [rnd.choice(distinct) for _ in range(T + 1)]
    w = key_rows(ctx, keys)
    (asc, want), _ = both_directions(ctx, w, (b"k",), "classes")
    assert SW.refine([k.encode() for k in keys])[1] == 2 and len(set(want.values)) > 250


# ---- 3. statuses, the empty path ------------------------------------------------------------------------------------------------------------
def test_every_status(ctx):
    rows = ['{"k":"b"}', '{"x":1}', '7', '{"k":"a"}', '{"k":null}', '{"k":12}', '{"k":true}', '{"k":{"k":"a"}}', '{"k":[1]}', '{"k":""}', '{"k":"a"}',
            '{"k":1.5}', '"k"', '{"k":"b"}']
    w, sel = array_rows(ctx, rows)
    for desc in (False, True):
        ctx.select_rows((b"rows",))
        got, want = check_order(ctx, w, sel, (b"k",), desc, 0, "statuses")
        assert got.order.tolist()[5:] == [1, 2, 4, 5, 6, 7, 8, 11, 12]  # last, in row order, in both directions
        assert got.status.tolist()[5:] == [CW.COL_NOT_FOUND, CW.COL_NOT_OBJECT, CW.COL_NULL] + [CW.COL_TYPE] * 5 + [CW.COL_NOT_OBJECT]
        assert got.order.tolist()[:5] == ([0, 13, 3, 10, 9] if desc else [9, 3, 10, 0, 13])
    w = oracle_walk(STATUS_DOC, False, True)
    ctx.parse(STATUS_DOC)
    sel = RW.select_rows(w, (b"rows",))
    for path in ((b"k",), (b"nope",), (b"v",)):
        ctx.select_rows((b"rows",))
        check_order(ctx, w, sel, path, True, 0, "the status document")
    ctx.select_records()


def test_empty_path_over_scalar_rows(ctx):
    doc = b'{"n":["pear",3,"apple","",null,"pear",["x"],"fig"]}'
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = RW.select_rows(w, (b"n",))
    ctx.select_rows((b"n",))
    got, _ = check_order(ctx, w, sel, (), False, 0, "scalars")
    assert got.order.tolist() == [3, 2, 7, 0, 5, 1, 4, 6] and got.status.tolist() == [0] * 5 + [CW.COL_TYPE, CW.COL_NULL, CW.COL_TYPE]
    got, want = check_order(ctx, w, sel, (), True, 3, "scalars, top 3")
    assert want.values == [b"pear", b"pear", b"fig"] and got.order.tolist() == [0, 1, 2]
    ctx.select_records()


# ---- 4. limits --------------------------------------------------------------------------------------------------------------------------
def limit_lines():
    # every 11th row has no OK key; the others repeat 50 keys: every limit falls into a run of equal keys
    return ['{"v":%s}' % ("17" if r % 11 == 10 else '"name %02d"' % ((r * 7) % 50)) for r in range(N_LIMIT)]


@pytest.mark.parametrize("limit", [1, T, T + 1, N_OK - 1, N_OK, N_OK + 1, N_LIMIT - 1, N_LIMIT, N_LIMIT + 5, 0])
def test_limits(ctx, limit):
    w = nd_rows(ctx, limit_lines())
    (asc, want), (desc, _) = both_directions(ctx, w, (b"v",), "limit", limit)
    assert asc.rows == (N_LIMIT if limit == 0 or limit >= N_LIMIT else limit)
    assert want.status.count(OK) == min(asc.rows, N_OK)


def test_equal_keys_across_the_limit(ctx):
    w, sel = array_rows(ctx, ['{"k":"%s"}' % k for k in ["m", "b", "m", "m", "a", "m", "m", "x"]])
    got, want = check_order(ctx, w, sel, (b"k",), False, 4, "ties")
    assert got.order.tolist() == [3, 1, 0, 2] and want.selection[0] == [0, 4]  # rows 4, 1 and the first two of the five "m"
    ctx.select_rows((b"rows",))
    got, want = check_order(ctx, w, sel, (b"k",), True, 3, "ties, descending")
    assert got.order.tolist() == [2, 0, 1] and want.values == [b"x", b"m", b"m"]  # row 7, then the first two "m" in row order
    ctx.select_records()


# ---- 5. scans beyond one tile -------------------------------------------------------------------------------------------------------------
def test_seventy_thousand_rows(ctx):
    """70 000 rows, two thirds of them distinct, lengths 0 .. 20: 69 tiles in every scan of a round, three rounds."""
    rnd = random.Random(70)
    n = 70000
    pool = ["".join(rnd.choice("abcxyz01") for _ in range(rnd.randrange(21))) for _ in range(100)]
    keys = [pool[rnd.randrange(100)] if r % 3 == 0 else "".join(rnd.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randrange(21))) for r in range(n)]
    w = nd_rows(ctx, ['{"v":%s}' % ("null" if r % 997 == 0 else js(k)) for r, k in enumerate(keys)])
    got, want = check_order(ctx, w, None, (b"v",), False, 0, "70000")
    assert got.rows == n and len(set(want.values)) > n // 2
    ctx.select_records()
    got, want = check_order(ctx, w, None, (b"v",), True, 1000, "70000, the largest 1000")
    assert got.rows == 1000
    ctx.select_records()


# ---- 6. composition -----------------------------------------------------------------------------------------------------------------------
ITEM_LINES = ['{"items":[{"id":1,"v":"d"},{"id":2,"v":"k"},{"id":3,"v":"a"}]}', '{"items":[]}', '{"x":1}', '{"items":[{"id":4,"v":"h"}]}', '{"items":7}',
              '{"items":[{"id":5,"v":"i"},{"id":6,"v":"b"},{"id":7},{"id":8,"v":"i"},{"id":9,"v":""}]}', '{"items":[{"id":10,"v":"c"}]}']


@pytest.mark.parametrize("limit", [0, 1, 4, 7, 10, 50])
def test_records_that_own_no_one_and_many_rows(ctx, limit):
    doc = "\n".join(ITEM_LINES).encode()
    w = oracle_walk(doc, True, True)
    for desc in (False, True):
        ctx.parse(doc, ndjson=True)
        sel = RW.select_rows(w, (b"items",))
        assert ctx.select_rows((b"items",)) == (7, 10)
        got, want = check_order(ctx, w, sel, (b"v",), desc, limit, "items")
        assert want.selection[2] == sel[2] and got.records == 7
        check_order(ctx, w, want.selection, (b"v",), not desc, 3, "items, again")  # a second order on what the first left
    ctx.select_records()


@pytest.mark.parametrize("copy", [True, False], ids=["copied", "in-the-message"])
def test_with_a_row_predicate_in_front_and_behind(ctx, copy):
    rows = ['{"id":%d,"v":"name %03d","t":"%s"}' % (r, (r * 37) % 101, "ab"[r % 2]) for r in range(300)]
    w, sel = array_rows(ctx, rows, copy=copy)
    narrowed = WW.where(w, sel, (b"t",), Q.OP_EQ_STRING, b"a")
    assert ctx.where_path((b"t",), ctx.OP_EQ_STRING, b"a") == (1, 150)
    got, want = check_order(ctx, w, narrowed, (b"v",), True, 20, "where, then order")
    after = WW.where(w, want.selection, (b"id",), WW.OP_GE_INT, 150)
    assert ctx.where_path((b"id",), ctx.OP_GE_INT, 150) == (1, len(after[1]))
    same_selection(ctx, 1, len(after[1]), after, "order, then where")
    check_order(ctx, w, after, (b"v",), False, 2, "and order again")
    ctx.select_records()


def test_behind_an_unnest_on_twitter_hashtags(ctx):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = RW.select_rows(w, (b"statuses",))
    assert ctx.select_rows((b"statuses",)) == (1, len(sel[1]))
    offs, index, sts = UW.unnest_rows(RW.RowWalk(w, sel[1]), (b"entities", b"hashtags"), sel[0], sel[2])[:3]
    assert ctx.unnest_rows((b"entities", b"hashtags"))[2] == len(index) >= 2  # (few statuses carry hashtags)
    for desc in (False, True):
        got, want = check_order(ctx, w, (offs, index, sts), (b"text",), desc, 0, "hashtags")
        assert set(want.status) == {OK}
    ctx.select_records()


TEXT_ROWS = ['{"id":%d,"v":"%s","n":%d}' % (r, "key %02d" % ((r * 61) % 97), r % 7) for r in range(200)]


@pytest.mark.parametrize("copy", [True, False], ids=["copied", "in-the-message"])
def test_the_consumers_of_the_selection_see_the_kept_rows(ctx, copy):
    k = 10
    w, sel = array_rows(ctx, TEXT_ROWS, copy=copy)
    got, want = check_order(ctx, w, sel, (b"v",), True, k, "top k")  # (check_order: extract_path_strings through order)
    by_key = sorted(range(200), key=lambda r: (-((r * 61) % 97), r))[:k]  # (200 rows over 97 keys: ties, in row order)
    n, text, off = ctx.marshal_rows(offsets=True)
    lines = [text[int(off[i]):int(off[i + 1]) - 1] for i in range(n)]
    assert n == k and [lines[i] for i in got.order.tolist()] == [TEXT_ROWS[r].encode() for r in by_key]
    want_text, want_off = MW.marshal_rows(w, want.selection[1])
    assert text == want_text and off.tolist() == [int(x) for x in want_off]
    (ids, st), (soff, sdata, sst) = ctx.extract_table([((b"id",), I), ((b"v",), ctx.COL_STRING)])
    assert ids[got.order.astype(np.int64)].tolist() == by_key and st.tolist() == [0] * k
    names = [sdata[int(a):int(b)] for a, b in zip(soff[:-1], soff[1:])]
    assert [names[i] for i in got.order.tolist()] == want.values
    agg = ctx.aggregate_path((b"id",), I)
    assert (agg.rows, agg.max, agg.min) == (k, max(by_key), min(by_key))
    if copy:  # filter_rows: the kept rows as a result of their own, in selection order
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
    got, want = check_order(ctx, w, sel, (b"user", b"screen_name"), False, 0, "screen names")
    assert set(want.status) == {OK} and want.values == sorted(want.values) and got.rows == len(sel[1])
    got, want = check_order(ctx, w, sel, (b"created_at",), True, 5, "the five latest dates as text")
    assert got.rows == 5 and want.values == sorted(want.values, reverse=True)
    n, text = ctx.marshal_rows()
    assert n == 5 and text == MW.marshal_rows(w, want.selection[1])[0]
    ctx.select_records()


def test_parking_by_make(ctx):
    doc = b"\n".join(workloads.c5_parking_nd(3).split(b"\n")[:3000])
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    assert len(w.records()) == 3000
    (asc, want), _ = both_directions(ctx, w, (b"Make",), "parking")
    assert set(want.status) == {OK} and max(map(len, want.values)) < 7  # short keys, many duplicates: one round
    both_directions(ctx, w, (b"IssueData",), "parking dates", 10)  # 19 bytes, a shared prefix: three rounds


# ---- 7. lifecycle, errors -------------------------------------------------------------------------------------------------------------------
def same_order(a, b):
    assert (a.records, a.rows, a.kind) == (b.records, b.rows, b.kind)
    assert np.array_equal(a.order, b.order) and np.array_equal(a.status, b.status)
    assert (a.values is None and b.values is None) or np.array_equal(a.values, b.values)


def test_lifecycle(ctx):
    import sjhip
    L = sjhip.lib()
    doc = fixtures.load("twitter")
    ctx.trim()
    ctx.parse(doc, key_flags=True)
    ctx.select_rows((b"statuses",))
    before = ctx.device_bytes()
    first = ctx.order_path_strings((b"user", b"screen_name"), descending=True, limit=30)
    assert ctx.device_bytes() > before and first.kind == S and first.values is None
    ctx.select_rows((b"statuses",))
    same_order(ctx.order_path_strings((b"user", b"screen_name"), descending=True, limit=30), first)  # the same bits again
    # a non-NULL values after a string order: an argument error that says why, and the order stays
    buf = np.zeros(30, dtype=np.uint64)
    assert L.sjhip_fetch_order(ctx._h, None, buf.ctypes.data, None) == ERR_ARG
    assert "no 8-byte values" in ctx.last_error() and "sjhip_extract_path_strings" in ctx.last_error()
    same_order(ctx.fetch_order(sjhip.Order(1, 30, S)), first)
    # a numeric order replaces it, and a string order replaces that
    ctx.select_rows((b"statuses",))
    numeric = ctx.order_path((b"retweet_count",), I, descending=True, limit=7)
    assert numeric.kind == I and numeric.values.dtype == np.int64 and L.sjhip_fetch_order(ctx._h, None, buf.ctypes.data, None) == 0
    ctx.select_rows((b"statuses",))
    again = ctx.order_path_strings((b"user", b"screen_name"), descending=True, limit=30)
    same_order(again, first)
    sel = ctx.fetch_rows(1, 30)
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
    same_order(ctx.fetch_order(sjhip.Order(1, 30, S)), first)
    # ... and they survive it
    ctx.select_rows((b"statuses",))
    groups = ctx.group_path((b"lang",), ctx.COL_STRING, (b"retweet_count",), I, fetch=False)
    column = ctx.extract_path_strings((b"lang",), fetch=False)
    marshaled = ctx.marshal_rows()
    ctx.order_path_strings((b"lang",), limit=7)
    kept = ctx.fetch_rows(1, 7)
    g = ctx.fetch_groups(groups)
    assert sorted(g.keys) == [b"ja", b"zh"] and len(ctx.fetch_path_strings(*column)[1]) == 200
    out_text = np.empty(len(marshaled[1]), dtype=np.uint8)
    assert marshaled[0] == 100 and L.sjhip_fetch_marshaled_rows(ctx._h, None, out_text.ctypes.data) == 0 and out_text.tobytes() == marshaled[1]
    assert ctx.marshal_rows(fetch=False)[0] == 7 and ctx.marshal_json() == text
    # errors in the checks touch nothing: the selection and the order are bit for bit as before
    previous = ctx.fetch_order(sjhip.Order(1, 7, S))
    nr, nw = C.c_size_t(77), C.c_size_t(77)
    lens = (C.c_uint32 * 1)(4)
    out = (C.byref(nr), C.byref(nw))
    for flags, word in [(2, "flag bits 0x2"), (0x80000001, "flag bits 0x80000000")]:
        assert L.sjhip_order_path_strings(ctx._h, b"lang", lens, 1, flags, 3, *out) == ERR_ARG
        assert word in ctx.last_error() and (nr.value, nw.value) == (77, 77), ctx.last_error()
    with pytest.raises(sjhip.ParseError):
        ctx.order_path_strings((b"k",) * 17)  # a path longer than sjhip_find_path takes
    assert L.sjhip_order_path_strings(ctx._h, None, None, 1, 0, 0, *out) == ERR_ARG and ctx.last_error()  # keys announced, none given
    assert L.sjhip_order_path_strings(ctx._h, b"lang", lens, 1, 0, 0, None, None) == ERR_ARG and "null" in ctx.last_error()
    same_order(ctx.fetch_order(sjhip.Order(1, 7, S)), previous)
    for a, b in zip(ctx.fetch_rows(1, 7), kept):
        assert np.array_equal(a, b)
    # a selection without rows: nothing is launched, an empty order is published and fetched
    assert ctx.where_path((b"lang",), ctx.OP_EQ_STRING, b"en") == (1, 0)
    empty = ctx.order_path_strings((b"lang",), descending=True, limit=3)
    assert (empty.records, empty.rows, len(empty.order), empty.values, len(empty.status)) == (1, 0, 0, None, 0)
    assert ctx.fetch_rows(1, 0)[0].tolist() == [0, 0]
    ctx.select_records()
    # a parse drops it; so does a trim, which frees its arena
    ctx.parse(b'{"a":"x"}')
    assert L.sjhip_fetch_order(ctx._h, None, None, None) == ERR_ARG and "no order" in ctx.last_error()
    one = ctx.order_path_strings((b"a",))
    assert (one.records, one.rows, one.order.tolist(), one.status.tolist()) == (1, 1, [0], [0])
    ctx.trim()
    assert ctx.device_bytes() == 0 and L.sjhip_fetch_order(ctx._h, None, None, None) == ERR_ARG
    fresh = sjhip.Context(0)  # no result on the device
    assert L.sjhip_order_path_strings(fresh._h, b"lang", lens, 1, 0, 0, *out) == ERR_ARG and fresh.last_error()
    fresh.close()


def test_sharded_result_is_refused(ctx):
    import sjhip
    pad = "x" * 230
    doc = "\n".join('{"pad":"%s","k":"%d"}' % (pad, r % 7) for r in range(11000)).encode()
    assert len(doc) > 5 << 19
    many = sjhip.Context(0)
    try:
        with fixtures.nd_shard_limits(2 << 20, 1 << 20):
            many.parse(doc, ndjson=True)
        with pytest.raises(sjhip.ParseError):
            many.order_path_strings((b"k",))
        assert "is sharded" in many.last_error()
        assert many.aggregate_path((b"k",), I).status[CW.COL_TYPE] == 11000  # the result is as it was
    finally:
        many.close()
