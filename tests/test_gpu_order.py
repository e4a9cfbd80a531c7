"""GPU: the ordering (sjhip_order_path / sjhip_fetch_order) against the serial restatement of tests/order_walk.py over the oracle's
parse: on row counts around the wave and the sort tile (T = ORDER_SORT_TILE rows) with equal, ascending, descending, alternating and
random keys of the three kinds in both directions; with keys that differ in one byte, in two and in all eight (the pass plan); on
the edge keys of every kind; on every status; on limits around the tile, the OK rows and the row count; on 70 000 rows; under a
selection, under NDJSON records that own 0, 1 and many rows, before and behind a row predicate, and in front of the consumers of a
selection; and through the lifecycle and the error paths.

Everything is compared exactly: *records, *rows, the narrowed selection as sjhip_fetch_rows returns it (row offsets, row index,
statuses), order, the values as bit patterns, and the status bytes."""
import ctypes as C
import random

import numpy as np
import pytest

import column_walk as CW
import filter_rows_walk as FW
import fixtures
import marshal_rows_walk as MW
import order_walk as OW
import query_walk as Q
import rows_walk as RW
import where_walk as WW
from test_group_walk import STATUS_DOC
from test_gpu_columns import oracle_walk
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

F, I, U = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT
T = OW.ORDER_SORT_TILE
ERR_ARG = 5
DTYPE = {F: np.float64, I: np.int64, U: np.uint64}
U64 = (1 << 64) - 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_selection(ctx, records, rows, sel, what=None):
    off, idx, st = ctx.fetch_rows(records, rows)
    assert off.tolist() == [int(o) for o in sel[0]] and idx.tolist() == [int(i) for i in sel[1]] and st.tolist() == list(sel[2]), what


def check_order(ctx, w, sel, path, kind, descending=False, limit=0, what=None):
    """order_path on the selection in force (sel: the checker's copy of it, None: no selection) equals the checker.
    -> (what the device returned, the checker's Ordering: its .selection is the selection in force from here on)"""
    what = (what, path, kind, descending, limit)
    want = OW.order(w, sel, path, kind, descending, limit)
    got = ctx.order_path(path, kind, descending=descending, limit=limit)
    print(what, "records:", got.records, "rows:", got.rows, "passes:", bin(OW.pass_mask(want.values, want.status, kind, descending)).count("1"))
    assert (got.records, got.rows) == (want.records, want.rows), what
    same_selection(ctx, got.records, got.rows, want.selection, what)
    assert got.order.dtype == np.uint64 and got.order.tolist() == want.order, what
    assert got.values.dtype == DTYPE[kind] and bits(got.values).tolist() == want.values, what
    assert got.status.dtype == np.uint8 and got.status.tolist() == want.status, what
    assert sorted(got.order.tolist()) == list(range(got.rows)), what  # a permutation
    return got, want


def nd_rows(ctx, lines):
    """the lines as an ND document without a selection: the rows are the records"""
    doc = "\n".join(lines).encode()
    ctx.parse(doc, ndjson=True)
    return oracle_walk(doc, True, True)


def array_rows(ctx, rows, copy=True):
    """{"rows":[...]} with the selection on "rows" -> (walk, the selection)"""
    doc = ('{"rows":[%s]}' % ",".join(rows)).encode()
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy)
    sel = RW.select_rows(w, (b"rows",))
    assert ctx.select_rows((b"rows",)) == (1, len(sel[1])) and len(sel[1]) == len(rows)
    return w, sel


def all_directions(ctx, w, path, kind, what, limit=0):
    """on the records of an ND document: ascending and descending, each from no selection"""
    out = []
    for desc in (False, True):
        ctx.select_records()
        out.append(check_order(ctx, w, None, path, kind, desc, limit, what))
    ctx.select_records()
    return out


# ---- 1. shapes: the wave, the tile, five key patterns, three kinds, two directions -------------------------------------------------------
def random_float(rnd):
    while True:
        x = np.array([rnd.getrandbits(64)], dtype=np.uint64).view(np.float64)[0]
        if np.isfinite(x):
            return repr(float(x))


PATTERNS = {
    "all-equal": lambda r, n, rnd: ("7", "7", "7.5"),
    "ascending": lambda r, n, rnd: (str(r - 5), str(r), "%d.25" % (r - 5)),
    "descending": lambda r, n, rnd: (str(n - r - 5), str(n - r), "%d.25" % (n - r - 5)),
    "two-alternating": lambda r, n, rnd: (("5", "-3")[r % 2], ("5", "3")[r % 2], ("0.5", "-1e300")[r % 2]),
    "random-64-bit": lambda r, n, rnd: (str(rnd.randrange(-(1 << 63), 1 << 63)), str(rnd.getrandbits(64)), random_float(rnd)),
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_shapes(ctx, n, pattern):
    rnd = random.Random(n)
    w = nd_rows(ctx, ['{"i":%s,"u":%s,"f":%s}' % PATTERNS[pattern](r, n, rnd) for r in range(n)])
    for path, kind in (((b"i",), I), ((b"u",), U), ((b"f",), F)):
        (asc, _), (desc, _) = all_directions(ctx, w, path, kind, (pattern, n))
        if pattern == "all-equal":  # no pass: the order is the identity in both directions
            assert asc.order.tolist() == list(range(n)) == desc.order.tolist()
        if pattern == "two-alternating" and n > 1:  # stability across waves and rounds: each key's rows in row order
            assert asc.order.tolist() == list(range(1, n, 2)) + list(range(0, n, 2))
            assert desc.order.tolist() == list(range(0, n, 2)) + list(range(1, n, 2))


# ---- 1b. rows without a key at the seams: they travel through the sort as the missing bit of the class key ------------------------------
LACKING = {
    "every-third-lacks": lambda r, n: r % 3 != 2,
    "only-row-0-has": lambda r, n: r == 0,
    "only-the-last-has": lambda r, n: r == n - 1,
    "none-has": lambda r, n: False,
}


def lacking_cut(has):
    """a limit that cuts inside the block of rows without a key (the whole of it where it has one row)"""
    missing = has.count(False)
    return max(1, has.count(True) + (missing + 1) // 2)


@pytest.mark.parametrize("pattern", sorted(LACKING))
@pytest.mark.parametrize("n", [1, 2, 64, 65, OW.QTILE, OW.QTILE + 1])
def test_rows_without_a_key_at_the_seams(ctx, n, pattern):
    has = [LACKING[pattern](r, n) for r in range(n)]
    # (the keys repeat, so rows tie; a row without one lacks the member, or holds a null or a string)
    lines = ['{"i":%d,"u":%d,"f":%d.5}' % ((r * 7) % 5 - 2, (r * 7) % 5, (r * 7) % 5 - 2) if has[r] else
             ('{"x":%d}' % r, '{"i":null,"u":null,"f":null}', '{"i":"1","u":"1","f":"1"}')[r % 3] for r in range(n)]
    w = nd_rows(ctx, lines)
    for path, kind in (((b"i",), I), ((b"u",), U), ((b"f",), F)):
        for limit in (0, lacking_cut(has)):
            for got, want in all_directions(ctx, w, path, kind, (pattern, n), limit):
                kept = n if limit == 0 else min(n, limit)
                tail = kept - min(kept, has.count(True))  # the kept rows without a key: behind the others, in row order
                assert got.rows == kept and [st != CW.COL_OK for st in got.status.tolist()] == [False] * (kept - tail) + [True] * tail
                assert got.order.tolist()[kept - tail:] == sorted(got.order.tolist()[kept - tail:])
                assert all(v == 0 for v, st in zip(bits(got.values).tolist(), got.status.tolist()) if st != CW.COL_OK)


# ---- 2. one pass at a time ------------------------------------------------------------------------------------------------------------
DIGIT_SETS = [(d,) for d in range(8)] + [(0, 2), (1, 7), (3, 5)] + [tuple(range(8))]


@pytest.mark.parametrize("digits", DIGIT_SETS, ids=lambda ds: "digits-" + "".join(map(str, ds)))
def test_keys_that_differ_in_these_bytes_only(ctx, digits):
    rnd = random.Random(len(digits) * 8 + digits[0])
    n, base = T + 77, 0x4142434445464748
    keys = []
    for r in range(n):
        k = base
        for d in digits:
            k = (k & ~(0xFF << 8 * d)) | (rnd.randrange(256) << 8 * d)
        keys.append(k)
    w = nd_rows(ctx, ['{"k":%d}' % k for k in keys])
    mask = OW.pass_mask(keys, [CW.COL_OK] * n, U)
    assert mask == sum(1 << d for d in digits)  # the plan the device derives from the same keys: these passes and no other
    (asc, want), _ = all_directions(ctx, w, (b"k",), U, digits)
    assert asc.values.tolist() == sorted(keys)


# ---- 3. edge keys ---------------------------------------------------------------------------------------------------------------------
EDGE = {
    "int": (I, ["-9223372036854775808", "9223372036854775807", "0", "-1", "1", "-9223372036854775807", "9223372036854775806", "-1", "0"]),
    "uint": (U, ["9223372036854775808", "18446744073709551615", "0", "9223372036854775807", "18446744073709551614", "1", "9223372036854775808"]),
    "float": (F, ["0.0", "-0.0", "5e-324", "-5e-324", "1e308", "-1e308", "2.2250738585072014e-308", "-0.0", "0.0", "1.7976931348623157e308"]),
    "mixed-under-float": (F, ["1", "1.0", "0", "-0.0", "0.0", "18446744073709551615", "-9223372036854775808", "2.5", "2", "1e0"]),
    "truncated-to-equal-int": (I, ["1.9", "1", "1.0", "1.5", "-0.5", "0", "0.99", "-1.9", "-1", "9223372036854775808.0", "1e300"]),
    "uint-from-others": (U, ["-1", "1.5", "1", "18446744073709551616.0", "-0.0", "0", "1e30"]),
}


@pytest.mark.parametrize("case", sorted(EDGE))
@pytest.mark.parametrize("copy", [True, False], ids=["copied", "in-the-message"])
def test_edge_keys(ctx, case, copy):
    kind, values = EDGE[case]
    w, sel = array_rows(ctx, ['{"k":%s}' % v for v in values], copy=copy)
    got, want = check_order(ctx, w, sel, (b"k",), kind, False, 0, case)
    ctx.select_rows((b"rows",))
    desc, _ = check_order(ctx, w, sel, (b"k",), kind, True, 0, case)
    if case == "float":  # -0.0 below +0.0, each pair in row order
        assert got.order.tolist() == [5, 3, 1, 7, 0, 8, 2, 6, 4, 9] and desc.order.tolist() == [9, 4, 6, 2, 0, 8, 1, 7, 3, 5]
    if case == "truncated-to-equal-int":  # 1.9, 1, 1.0, 1.5 are the key 1; 2^63 as a float is MinInt64; 1e300 is RANGE
        assert got.order.tolist() == [9, 7, 8, 4, 5, 6, 0, 1, 2, 3, 10] and got.status.tolist() == [0] * 10 + [CW.COL_RANGE]
    ctx.select_records()


# ---- 4. every status ------------------------------------------------------------------------------------------------------------------
def test_every_status(ctx):
    w = oracle_walk(STATUS_DOC, False, True)
    ctx.parse(STATUS_DOC)
    sel = RW.select_rows(w, (b"rows",))
    for path, kind in (((b"v",), F), ((b"k",), I), ((b"nope",), U)):
        for desc in (False, True):
            ctx.select_rows((b"rows",))
            got, want = check_order(ctx, w, sel, path, kind, desc, 0, "statuses")
            tail = [r for r in range(13) if want.status[got.order.tolist().index(r)] != CW.COL_OK]
            assert got.order.tolist()[13 - len(tail):] == tail  # the rows without an OK key: last, in row order, in both directions
    ctx.select_rows((b"rows",))
    got, _ = check_order(ctx, w, sel, (b"k",), I, True, 0, "statuses")
    assert got.order.tolist() == [5, 11, 0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 12] and sorted(set(got.status.tolist())) == [0, 1, 2, 3, 4, 5]
    assert got.values.tolist() == [12, 12] + [0] * 11
    ctx.select_records()


# ---- 5. limits ------------------------------------------------------------------------------------------------------------------------
N_LIMIT = 2 * T + 3


def limit_lines():
    # every 11th row has no OK key; the others repeat 50 keys: every limit falls into a run of equal keys
    return ['{"v":%s}' % ('"x"' if r % 11 == 10 else str((r * 7) % 50 - 20)) for r in range(N_LIMIT)]


N_OK = N_LIMIT - N_LIMIT // 11


@pytest.mark.parametrize("limit", [1, T, T + 1, N_OK - 1, N_OK, N_OK + 1, N_LIMIT - 1, N_LIMIT, N_LIMIT + 5, 0])
def test_limits(ctx, limit):
    w = nd_rows(ctx, limit_lines())
    for kind in (I, F):
        (asc, want), (desc, _) = all_directions(ctx, w, (b"v",), kind, "limit", limit)
        assert asc.rows == (N_LIMIT if limit == 0 or limit >= N_LIMIT else limit)
        assert want.status.count(CW.COL_OK) == min(asc.rows, N_OK)


def test_equal_keys_across_the_limit(ctx):
    w, sel = array_rows(ctx, ['{"k":%d}' % k for k in [5, 1, 5, 5, 0, 5, 5, 9]])
    got, want = check_order(ctx, w, sel, (b"k",), U, False, 4, "ties")
    assert got.order.tolist() == [3, 1, 0, 2] and want.selection[0] == [0, 4]  # rows 4, 1 and the first two of the five 5s
    ctx.select_rows((b"rows",))
    got, want = check_order(ctx, w, sel, (b"k",), U, True, 3, "ties, descending")
    assert got.order.tolist() == [2, 0, 1] and got.values.tolist() == [9, 5, 5]  # row 7, then the first two 5s in row order
    ctx.select_records()
    # a whole tile of equal keys in front of keys that vary, cut inside the tile and behind it
    w = nd_rows(ctx, ['{"k":%d}' % (5 if r < T else r % 9) for r in range(2 * T + 3)])
    for limit in (T // 2, T + 10):
        for desc in (False, True):
            ctx.select_records()
            check_order(ctx, w, None, (b"k",), I, desc, limit, "an equal tile")
    ctx.select_records()


# ---- 6. scans beyond one tile -----------------------------------------------------------------------------------------------------------
def test_seventy_thousand_rows(ctx):
    """70 000 rows: 69 tiles of QTILE rows in the compaction scan and in the flag scan, 69 sort tiles and with them 256 * 69 = 17 664
    histogram entries, 18 tiles of the histogram scan.  The top level of every scan is k_tw_scan_sums, ONE block of 1024 threads
    that walks any number of tile sums in a loop (16 waves, each over a contiguous range): there is no row count at which it would
    need a second block.  What bounds it is the 2^30 rows of the call -- 2^20 tile sums of the row scans, 2^28 histogram entries and
    so 2^18 tile sums of the histogram scan --, which one block walks in a loop as well; that count cannot be run in seconds and is
    not run here (Order)."""
    rnd = random.Random(70)
    n = 70000
    lines = ['{"v":%s}' % ("null" if r % 997 == 0 else str(rnd.randrange(-(1 << 40), 1 << 40) if r % 3 else rnd.randrange(100))) for r in range(n)]
    w = nd_rows(ctx, lines)
    assert len(lines) > 64 * OW.QTILE and 256 * ((n + T - 1) // T) > 16 * OW.QTILE
    got, want = check_order(ctx, w, None, (b"v",), I, False, 0, "70000")
    assert got.rows == n and OW.pass_mask(want.values, want.status, I) == 0xFF  # both signs: the sign digit varies as well
    ctx.select_records()
    got, want = check_order(ctx, w, None, (b"v",), I, True, 1000, "70000, the largest 1000")
    assert got.rows == 1000
    ctx.select_records()


# ---- 7. composition ---------------------------------------------------------------------------------------------------------------------
ITEM_LINES = ['{"items":[{"id":1,"v":4},{"id":2,"v":9},{"id":3,"v":1}]}', '{"items":[]}', '{"x":1}', '{"items":[{"id":4,"v":7}]}', '{"items":7}',
              '{"items":[{"id":5,"v":8},{"id":6,"v":2},{"id":7},{"id":8,"v":8},{"id":9,"v":-1}]}', '{"items":[{"id":10,"v":3}]}']


@pytest.mark.parametrize("limit", [0, 1, 4, 7, 10, 50])
def test_records_that_own_no_one_and_many_rows(ctx, limit):
    doc = "\n".join(ITEM_LINES).encode()
    w = oracle_walk(doc, True, True)
    for desc in (False, True):
        ctx.parse(doc, ndjson=True)
        sel = RW.select_rows(w, (b"items",))
        assert ctx.select_rows((b"items",)) == (7, 10)
        got, want = check_order(ctx, w, sel, (b"v",), I, desc, limit, "items")
        assert want.selection[2] == sel[2] and got.records == 7
        # a second order on what the first left, by another key
        check_order(ctx, w, want.selection, (b"id",), U, not desc, 3, "items, again")
    ctx.select_records()


@pytest.mark.parametrize("copy", [True, False], ids=["copied", "in-the-message"])
def test_with_a_row_predicate_in_front_and_behind(ctx, copy):
    rows = ['{"id":%d,"v":%d,"t":"%s"}' % (r, (r * 37) % 101, "ab"[r % 2]) for r in range(300)]
    w, sel = array_rows(ctx, rows, copy=copy)
    narrowed = WW.where(w, sel, (b"t",), Q.OP_EQ_STRING, b"a")
    assert ctx.where_path((b"t",), ctx.OP_EQ_STRING, b"a") == (1, 150)
    got, want = check_order(ctx, w, narrowed, (b"v",), F, True, 20, "where, then order")
    after = WW.where(w, want.selection, (b"v",), WW.OP_GE_INT, 95)
    assert ctx.where_path((b"v",), ctx.OP_GE_INT, 95) == (1, len(after[1]))
    same_selection(ctx, 1, len(after[1]), after, "order, then where")
    check_order(ctx, w, after, (b"id",), I, False, 2, "and order again")
    ctx.select_records()


TEXT_ROWS = ['{"id":%d,"v":%d,"s":"row %d"}' % (r, (r * 61) % 97, r) for r in range(200)]


@pytest.mark.parametrize("copy", [True, False], ids=["copied", "in-the-message"])
def test_the_consumers_of_the_selection_see_the_kept_rows(ctx, copy):
    k = 10
    w, sel = array_rows(ctx, TEXT_ROWS, copy=copy)
    got, want = check_order(ctx, w, sel, (b"v",), I, True, k, "top k")
    by_key = sorted(range(200), key=lambda r: (-((r * 61) % 97), r))[:k]  # (200 rows over 97 values: ties, in row order)
    # marshal_rows: the lines taken in `order` are the k texts in key order
    n, text, off = ctx.marshal_rows(offsets=True)
    lines = [text[int(off[i]):int(off[i + 1]) - 1] for i in range(n)]
    assert n == k and [lines[i] for i in got.order.tolist()] == [TEXT_ROWS[r].encode() for r in by_key]
    want_text, want_off = MW.marshal_rows(w, want.selection[1])
    assert text == want_text and off.tolist() == [int(x) for x in want_off]
    # a table and a column on the kept rows, taken in `order`
    (ids, st), (soff, sdata, sst) = ctx.extract_table([((b"id",), I), ((b"s",), ctx.COL_STRING)])
    assert ids[got.order.astype(np.int64)].tolist() == by_key and st.tolist() == [0] * k
    names = [sdata[int(a):int(b)] for a, b in zip(soff[:-1], soff[1:])]
    assert [names[i] for i in got.order.tolist()] == [b"row %d" % r for r in by_key]
    vals, vst = ctx.extract_path((b"v",), I)
    assert vals[got.order.astype(np.int64)].tolist() == got.values.tolist()
    # aggregate_path over the kept rows: max equals values[0] of the descending order, min its last
    agg = ctx.aggregate_path((b"v",), I)
    assert (agg.rows, agg.max, agg.min) == (k, int(got.values[0]), int(got.values[-1]))
    ctx.select_rows((b"rows",))
    asc, _ = check_order(ctx, w, sel, (b"v",), F, False, k, "bottom k")
    assert ctx.aggregate_path((b"v",), F).min == float(asc.values[0])
    if copy:  # filter_rows: the kept rows as a result of their own, in selection order
        tape, strings, skipped = FW.filter_rows(w, want.selection[1])
        ctx.select_rows((b"rows",))
        ctx.order_path((b"v",), I, descending=True, limit=k)
        n_rows, skipped_got, pj = ctx.filter_rows()
        assert (n_rows, skipped_got) == (k, skipped) and pj.Tape.tolist() == tape and pj.Strings.tobytes() == strings
    ctx.select_records()


def test_twitter_top_five_by_retweet_count(ctx):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = RW.select_rows(w, (b"statuses",))
    assert ctx.select_rows((b"statuses",)) == (1, len(sel[1]))
    counts, sts = RW.column(RW.RowWalk(w, sel[1]), (b"retweet_count",), I)
    assert set(sts) == {CW.COL_OK}
    top = sorted(range(len(counts)), key=lambda r: (-counts[r], r))[:5]  # the host sort
    got, want = check_order(ctx, w, sel, (b"retweet_count",), I, True, 5, "twitter")
    assert got.values.tolist() == [counts[r] for r in top] and [sorted(top)[i] for i in got.order.tolist()] == top
    n, text = ctx.marshal_rows()
    assert n == 5 and text == MW.marshal_rows(w, want.selection[1])[0]
    ctx.select_records()
    # the records themselves: one row, its own key
    got, want = check_order(ctx, w, None, (b"search_metadata", b"count"), U, False, 0, "the record")
    assert (got.records, got.rows, got.order.tolist(), got.values.tolist()) == (1, 1, [0], [100])
    ctx.select_records()


def test_empty_path_over_scalar_rows(ctx):
    doc = b'{"n":[3,3.5,"3",4,-4.0,null,3]}'
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = RW.select_rows(w, (b"n",))
    ctx.select_rows((b"n",))
    got, _ = check_order(ctx, w, sel, (), F, False, 0, "scalars")
    assert got.order.tolist() == [4, 0, 6, 1, 3, 2, 5] and got.status.tolist() == [0] * 5 + [CW.COL_TYPE, CW.COL_NULL]
    got, _ = check_order(ctx, w, sel, (), I, True, 3, "scalars, top 3")
    assert got.values.tolist() == [4, 3, 3] and got.order.tolist() == [2, 0, 1]
    ctx.select_records()


# ---- 8. lifecycle, errors -----------------------------------------------------------------------------------------------------------------
def same_order(a, b):
    assert (a.records, a.rows, a.kind) == (b.records, b.rows, b.kind)
    for x, y in ((a.order, b.order), (bits(a.values), bits(b.values)), (a.status, b.status)):
        assert np.array_equal(x, y)


def test_lifecycle(ctx):
    import sjhip
    L = sjhip.lib()
    doc = fixtures.load("twitter")
    ctx.trim()
    ctx.parse(doc, key_flags=True)
    ctx.select_rows((b"statuses",))
    before = ctx.device_bytes()
    first = ctx.order_path((b"user", b"followers_count"), U, descending=True, limit=30)
    assert ctx.device_bytes() > before  # the arena of the order is counted
    ctx.select_rows((b"statuses",))
    again = ctx.order_path((b"user", b"followers_count"), U, descending=True, limit=30)
    same_order(first, again)  # two calls on the same result return the same bits
    sizes = sjhip.Order(again.records, again.rows, U)
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
    same_order(ctx.fetch_order(sizes), first)
    # ... and they survive it: a grouping, a column, the text of the rows and the selection are as they were after an order call
    ctx.select_rows((b"statuses",))
    groups = ctx.group_path((b"lang",), ctx.COL_STRING, (b"retweet_count",), I, fetch=False)
    column = ctx.extract_path_strings((b"lang",), fetch=False)
    marshaled = ctx.marshal_rows()
    ctx.order_path((b"retweet_count",), I, limit=7)
    kept = ctx.fetch_rows(1, 7)
    g = ctx.fetch_groups(groups)
    assert sorted(g.keys) == [b"ja", b"zh"] and len(ctx.fetch_path_strings(*column)[1]) == 200
    buf = np.empty(len(marshaled[1]), dtype=np.uint8)
    assert marshaled[0] == 100 and L.sjhip_fetch_marshaled_rows(ctx._h, None, buf.ctypes.data) == 0 and buf.tobytes() == marshaled[1]
    assert ctx.marshal_rows(fetch=False)[0] == 7  # ... and a new text is of the kept rows
    assert ctx.marshal_json() == text
    # errors in the checks touch nothing: the selection and the order are bit for bit as before
    previous = ctx.fetch_order(sjhip.Order(1, 7, I))
    nr, nw = C.c_size_t(77), C.c_size_t(77)
    lens = (C.c_uint32 * 1)(13)
    out = (C.byref(nr), C.byref(nw))
    for kind, flags, word in [(3, 0, "key kind 3"), (4, 0, "key kind 4"), (99, 0, "key kind 99"), (-1, 0, "key kind -1"), (I, 2, "flag bits 0x2"),
                              (I, 0x80000001, "flag bits 0x80000000")]:
        assert L.sjhip_order_path(ctx._h, b"retweet_count", lens, 1, kind, flags, 3, *out) == ERR_ARG
        assert word in ctx.last_error() and (nr.value, nw.value) == (77, 77), ctx.last_error()
    with pytest.raises(sjhip.ParseError):
        ctx.order_path((b"k",) * 17, I)  # a path longer than sjhip_find_path takes
    assert L.sjhip_order_path(ctx._h, None, None, 1, I, 0, 0, *out) == ERR_ARG and ctx.last_error()  # keys announced, none given
    assert L.sjhip_order_path(ctx._h, b"retweet_count", lens, 1, I, 0, 0, None, None) == ERR_ARG and "null" in ctx.last_error()
    same_order(ctx.fetch_order(sjhip.Order(1, 7, I)), previous)
    for a, b in zip(ctx.fetch_rows(1, 7), kept):
        assert np.array_equal(a, b)
    assert L.sjhip_fetch_order(ctx._h, None, None, None) == 0  # every destination null
    # a selection without rows: nothing is launched, an empty order is published and fetched
    assert ctx.where_path((b"lang",), ctx.OP_EQ_STRING, b"en") == (1, 0)
    empty = ctx.order_path((b"retweet_count",), F, descending=True, limit=3)
    assert (empty.records, empty.rows, len(empty.order), len(empty.values), len(empty.status)) == (1, 0, 0, 0, 0)
    assert ctx.fetch_rows(1, 0)[0].tolist() == [0, 0]
    ctx.select_records()
    # a parse drops it; so does a trim, which frees its arena
    ctx.parse(b'{"a":1}')
    assert L.sjhip_fetch_order(ctx._h, None, None, None) == ERR_ARG and "no order" in ctx.last_error()
    one = ctx.order_path((b"a",), I)
    assert (one.records, one.rows, one.order.tolist(), one.values.tolist(), one.status.tolist()) == (1, 1, [0], [1], [0])
    ctx.trim()
    assert ctx.device_bytes() == 0
    assert L.sjhip_fetch_order(ctx._h, None, None, None) == ERR_ARG
    fresh = sjhip.Context(0)  # no result on the device
    assert L.sjhip_order_path(fresh._h, b"retweet_count", lens, 1, I, 0, 0, *out) == ERR_ARG and fresh.last_error()
    assert L.sjhip_fetch_order(fresh._h, None, None, None) == ERR_ARG and "no order" in fresh.last_error()
    fresh.close()


def test_sharded_result_is_refused(ctx):
    import sjhip
    pad = "x" * 230
    doc = "\n".join('{"pad":"%s","k":%d}' % (pad, r % 7) for r in range(11000)).encode()
    assert len(doc) > 5 << 19
    many = sjhip.Context(0)
    try:
        with fixtures.nd_shard_limits(2 << 20, 1 << 20):
            many.parse(doc, ndjson=True)
        with pytest.raises(sjhip.ParseError):
            many.order_path((b"k",), I)
        assert "sharded" in many.last_error()
        assert many.aggregate_path((b"k",), I).status[CW.COL_OK] == 11000  # the result is as it was
    finally:
        many.close()
