"""GPU: row predicates by membership in a set (sjhip_where_path_in, sjhip_count_where_path_in) against the serial restatement of
tests/where_in_walk.py over the oracle's parse: what fetch_rows delivers after the call and what the count says before it.  Every
set of 1 to 16 values whose strings fit sjhip_where_paths' 1024 value bytes also runs against sjhip_where_paths with the OR program
on the same context, bit for bit.  Set sizes around the capacity steps, constructed table placements (tests/group_table.py:
chains across the last slot, one 64-bit hash for several values, strangers inside a chain), string lengths around the 8-byte word,
the conversions of INT / UINT, the seams of the wave (64), the block (256) and the scan tile (1024), compositions, the round trip
from a grouping, the count, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import column_walk as CW
import fixtures
import query_walk as Q
import rows_walk as RW
import unnest_walk as UW
import where_in_walk as IW
import where_walk as WW
from test_gpu_columns import oracle_walk
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

S, I, U = IW.COL_STRING, CW.COL_INT, CW.COL_UINT
OK = 0
QTILE = 1024  # rows per scan tile of the narrowing (csrc/sj_tapewalk.h)
K = (b"k",)


def fetched(ctx, nr, rows):
    return [a.copy() for a in ctx.fetch_rows(nr, rows)]


def same_selection(a, b, what):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y), what


def check_in(ctx, w, sel, reselect, path, kind, values, negate=False):
    """where_path_in on the selection in force (sel: the walker's, None without one; reselect() puts it back in force) equals the
    walker, count_where_path_in counted the rows it keeps, and sjhip_where_paths with one EQ per value under OR keeps the same rows
    bit for bit where it can take the set; -> the walker's new selection"""
    values = list(values)
    want_off, want_idx, want_st = IW.where_in(w, sel, path, kind, values, negate)
    what = (path, kind, len(values), negate)
    assert ctx.count_where_path_in(path, kind, values, negate) == len(want_idx), what
    by_or = None
    if 1 <= len(values) <= 16 and (kind != S or sum(len(v) for v in values) <= 1024):
        preds = [(path, IW.EQ_OF[kind], s) for s in IW.set_values(kind, values)]
        program = bytes([0] + [x for p in range(1, len(preds)) for x in (p, 0x81)] + ([0x82] if negate else []))
        by_or = fetched(ctx, *ctx.where_paths(preds, program))
        reselect()
    nr, rows = ctx.where_path_in(path, kind, values, negate)
    assert (nr, rows) == (len(want_st), len(want_idx)), (what, nr, rows)
    got = fetched(ctx, nr, rows)
    off, idx, st = got
    assert off.dtype == np.uint64 and idx.dtype == np.uint64 and st.dtype == np.uint8
    assert st.tolist() == want_st and off.tolist() == want_off, what
    assert np.array_equal(idx, np.array(want_idx, dtype=np.uint64)), what
    if by_or is not None:
        same_selection(got, by_or, what)
    return want_off, want_idx, want_st


def nd(ctx, lines, copy=True):
    doc = "\n".join(lines).encode()
    w = oracle_walk(doc, True, copy)
    ctx.parse(doc, ndjson=True, copy_strings=copy)
    return w


def check_both(ctx, w, path, kind, values):
    """with and without SJHIP_WHERE_NOT on the records -> the rows kept without it"""
    kept = check_in(ctx, w, None, ctx.select_records, path, kind, values)
    ctx.select_records()
    rest = check_in(ctx, w, None, ctx.select_records, path, kind, values, negate=True)
    ctx.select_records()
    assert sorted(kept[1] + rest[1]) == [r + 1 for r in w.records()]
    return kept[1]


# ---- set sizes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [I, S], ids=["int", "str"])
def test_set_sizes(ctx, kind):
    key = (lambda r: str(r * 7 - 50)) if kind == I else (lambda r: '"key-%d"' % r)
    val = (lambda r: r * 7 - 50) if kind == I else (lambda r: b"key-%d" % r)
    w = nd(ctx, ['{"k":%s}' % key(r % 90) for r in range(200)])
    for values in ([], [val(3)], [val(3), val(500)], [val(r) for r in range(0, 64, 2)], [val(r) for r in range(0, 66, 2)],
                   [val(5)] * 100, [val(r) for r in range(40, 140)]):
        kept = check_both(ctx, w, K, kind, values)
        assert len(kept) == sum(val(r % 90) in values for r in range(200))
    assert IW.GT.capacity(32) == 64 and IW.GT.capacity(33) == 128 and len(range(0, 66, 2)) == 33  # the capacity step


def test_65536_int_values_against_4096_rows(ctx):
    w = nd(ctx, ['{"k":%d}' % (r * 3) for r in range(4096)])
    values = np.arange(65536, dtype=np.int64) * 2 - 1000  # the even numbers from -1000: every second row up to 130 070
    kept = check_in(ctx, w, None, ctx.select_records, K, I, values)
    assert len(kept[1]) == sum((r * 3) % 2 == 0 and r * 3 <= 130070 for r in range(4096)) > 1000
    ctx.select_records()


# ---- table placement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IW.families()))
def test_constructed_tables(ctx, name):
    f = IW.families()[name]
    w = nd(ctx, f.rows_json())
    kept = check_both(ctx, w, K, f.kind, f.values)
    roots = w.records()
    assert kept == [roots[r] + 1 for r, keep in enumerate(f.kept()) if keep], f.says


def test_constructed_tables_without_copied_strings(ctx):
    for name in ("collide19", "twins", "home63_str"):
        f = IW.families()[name]
        w = nd(ctx, f.rows_json(), copy=False)
        assert len(check_both(ctx, w, K, f.kind, f.values)) == sum(f.kept())


# ---- strings ------------------------------------------------------------------------------------------------------------------------
def text(n, salt):
    return bytes(IW.GT.ALPHABET[(salt + 7 * i) % 93] for i in range(n))


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_string_lengths(ctx, copy):
    short = [text(n, n) for n in (0, 7, 8, 9, 31, 32, 33)]
    long = text(1024, 5)
    rows = short + [long, text(1025, 5), text(5000, 5), long[:-1] + b"!", long[:-1], short[4][:-1] + b"!", short[6] + b"!", b"A", text(8, 1)]
    lines = ['{"k":"%s"}' % r.decode() for r in rows] + ['{"k":"\\u0041"}', '{"k":"%s\\u0041"}' % long[:-1].decode()]
    w = nd(ctx, lines, copy)
    n = len(lines)
    assert len(check_both(ctx, w, K, S, short)) == 7  # (against the OR program too: 120 value bytes)
    assert len(check_both(ctx, w, K, S, [long])) == 1  # ... 1024 value bytes, alone
    assert len(check_both(ctx, w, K, S, short + [long, b"A"])) == 10  # "A" and its escaped spelling
    assert len(check_both(ctx, w, K, S, [long[:-1] + b"A", b"\\u0041"])) == 1  # 1023 bytes and an escape that ends the string
    assert n == 18


# ---- INT and UINT ---------------------------------------------------------------------------------------------------------------------
NUMBER_ROWS = ["1", "1.0", "1.9", "-1", "-1.5", "9223372036854775808", "18446744073709551615", "9223372036854775808.0",
               "18446744073709551616.0", "null", '"1"', '{"k":1}', "[1]", "true", "0", "-0.0"]


def test_conversions_and_rows_without_a_key(ctx):
    lines = ['{"a":{"k":%s}}' % t for t in NUMBER_ROWS] + ['{"a":{"x":1}}', '{"a":5}', '{"b":1}', "[1]"]
    w = nd(ctx, lines)
    path = (b"a", b"k")
    assert len(check_both(ctx, w, path, I, [1])) == 3 and len(check_both(ctx, w, path, U, [1])) == 3
    assert len(check_both(ctx, w, path, I, [-1])) == 2 and len(check_both(ctx, w, path, U, [(1 << 64) - 1])) == 1
    for kind, kept in ((I, 3), (U, 3)):  # INT: the bits of 2^63 are MinInt64 (the float 2^63), those of 2^64 - 1 are -1
        assert len(check_both(ctx, w, path, kind, [1 << 63, (1 << 64) - 1])) == kept, kind
    assert len(check_both(ctx, w, path, U, [0])) == 3 and len(check_both(ctx, w, path, I, [0, 1, -1])) == 7


# ---- row counts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 256, 257, QTILE - 1, QTILE, QTILE + 1))
def test_row_counts_at_the_seams(ctx, n):
    w = nd(ctx, ['{"k":%d}' % r for r in range(n)])
    last_wave = list(range((n - 1) // 64 * 64, n))
    for values, kept in ((last_wave, len(last_wave)), ([-5, n], 0), (list(range(n)), n), ([n - 1], 1), ([0, n - 1, 1023, 1024], None)):
        got = check_in(ctx, w, None, ctx.select_records, K, I, values)
        assert kept is None or len(got[1]) == kept, (n, kept)
        ctx.select_records()
    got = check_in(ctx, w, None, ctx.select_records, K, I, [n - 1], negate=True)
    assert len(got[1]) == n - 1
    ctx.select_records()


# ---- composition ----------------------------------------------------------------------------------------------------------------------
def test_behind_select_rows_unnest_and_where_path(ctx):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    base = RW.select_rows(w, (b"statuses",))

    def statuses():
        ctx.select_rows((b"statuses",))

    statuses()
    sel = check_in(ctx, w, base, statuses, (b"lang",), S, [b"ja", b"en"])
    assert 0 < len(sel[1]) < len(base[1])

    def again():
        statuses()
        ctx.where_path_in((b"lang",), S, [b"ja", b"en"])

    sel2 = WW.where(w, sel, (b"retweet_count",), WW.OP_GE_INT, 1)  # in front of where_path ...
    assert ctx.where_path((b"retweet_count",), WW.OP_GE_INT, 1) == (len(sel2[2]), len(sel2[1]))
    ids = ctx.extract_path((b"user", b"id"), ctx.COL_INT)[0].tolist()

    def narrowed():
        again()
        ctx.where_path((b"retweet_count",), WW.OP_GE_INT, 1)

    sel3 = check_in(ctx, w, sel2, narrowed, (b"user", b"id"), I, ids[::2])  # ... and behind it
    assert 0 < len(sel3[1]) < len(sel2[1])
    # behind unnest_rows: the hashtags of the statuses, by their text
    statuses()
    tags = UW.unnest_rows(RW.RowWalk(w, base[1]), (b"entities", b"hashtags"), base[0], base[2])[:3]
    ctx.unnest_rows((b"entities", b"hashtags"))

    def unnested():
        statuses()
        ctx.unnest_rows((b"entities", b"hashtags"))

    texts = ctx.extract_path_strings((b"text",))
    some = sorted({bytes(texts[1][int(a):int(b)]) for a, b in zip(texts[0][:-1], texts[0][1:])})[::2]
    sel4 = check_in(ctx, w, tags, unnested, (b"text",), S, some)
    assert 0 < len(sel4[1]) < len(tags[1])
    ctx.select_records()


def test_without_a_selection_one_is_created_and_no_rows_launch_nothing(ctx):
    import sjhip
    w = nd(ctx, ['{"k":%d,"tags":["a","b","a",%d]}' % (r, r) for r in range(70)])
    with pytest.raises(sjhip.ParseError):
        ctx.fetch_rows(70, 70)
    sel = check_in(ctx, w, None, ctx.select_records, K, I, [3, 69, 500])
    assert sel == ([0] * 4 + [1] * 66 + [2], sel[1], [OK] * 70) and len(sel[1]) == 2
    none = check_in(ctx, w, sel, lambda: (ctx.select_records(), ctx.where_path_in(K, I, [3, 69, 500])), K, I, [4])
    assert none[1] == [] and none[0] == [0] * 71
    for values, negate in (([3], False), ([3], True), ([], True)):  # on the selection without rows nothing is launched
        assert check_in(ctx, w, none, lambda: (ctx.select_records(), ctx.where_path_in(K, I, [3, 69, 500]), ctx.where_path_in(K, I, [4])),
                        K, I, values, negate) == none
    # n_keys == 0 on scalar rows
    ctx.select_records()
    base = RW.select_rows(w, (b"tags",))
    ctx.select_rows((b"tags",))
    a = check_in(ctx, w, base, lambda: ctx.select_rows((b"tags",)), (), S, [b"a", b"zz"])
    assert len(a[1]) == 140 and a[0][:3] == [0, 2, 4]
    ctx.select_rows((b"tags",))
    b = check_in(ctx, w, base, lambda: ctx.select_rows((b"tags",)), (), I, [5, 6, 7], negate=True)
    assert len(b[1]) == 280 - 3
    ctx.select_records()


def test_other_products_survive(ctx):
    doc = fixtures.load("parking-citations")
    ctx.parse(doc, ndjson=True)
    g = ctx.group_path((b"Make",), S, (b"Agency",), ctx.COL_FLOAT)
    nr, nb = ctx.extract_table([((b"Make",), S), ((b"Agency",), ctx.COL_FLOAT)], fetch=False)
    cols = [ctx.fetch_table_column(0, nr, S, nb[0]), ctx.fetch_table_column(1, nr, ctx.COL_FLOAT)]
    assert ctx.where_path_in((b"Make",), S, g.keys[:5]) == (g.rows, int(g.group_rows[:5].sum()))
    g2 = ctx.fetch_groups(type(g)(g.rows, g.groups, g.key_bytes, g.key_kind, g.value_kind))
    assert g2.keys == g.keys
    for x, y in zip((g.first_row, g.group_rows, g.codes, g.status) + g.aggregates(), (g2.first_row, g2.group_rows, g2.codes, g2.status) + g2.aggregates()):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for c, (kind, want) in enumerate(zip((S, ctx.COL_FLOAT), cols)):
        got = ctx.fetch_table_column(c, nr, kind, nb[c]) if kind == S else ctx.fetch_table_column(c, nr, kind)
        for x, y in zip(got, want):
            assert (x == y) if isinstance(x, bytes) else np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    ctx.select_records()


# ---- the round trip the call exists for ---------------------------------------------------------------------------------------------
def test_the_three_largest_groups_passed_back(ctx):
    doc = fixtures.load("parking-citations")
    ctx.parse(doc, ndjson=True)
    g = ctx.group_path((b"Make",), S)
    top = np.argsort(-g.group_rows.astype(np.int64), kind="stable")[:3]
    offsets = np.zeros(4, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(g.keys[j]) for j in top])
    data = np.frombuffer(b"".join(g.keys[j] for j in top), dtype=np.uint8)
    count = ctx.count_where_path_in((b"Make",), S, (offsets, data))
    nr, rows = ctx.where_path_in((b"Make",), S, (offsets, data))
    in_top = np.isin(g.codes, top.astype(np.uint32))
    assert nr == g.rows and rows == count == int(in_top.sum()) == int(g.group_rows[top].sum()) > 0
    off, idx, st = ctx.fetch_rows(nr, rows)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(in_top)]).astype(np.uint64))  # exactly the rows whose code is one of the three
    # ... and the anti-join keeps the others; the keys as a list of bytes are the same set
    ctx.select_records()
    assert ctx.where_path_in((b"Make",), S, [g.keys[j] for j in top], negate=True) == (nr, g.rows - rows)
    ctx.select_records()


# ---- the count --------------------------------------------------------------------------------------------------------------------------
def test_the_count_touches_nothing(ctx):
    w = nd(ctx, ['{"items":[%s]}' % ",".join('{"k":"v%d"}' % ((r * 5 + j) % 9) for j in range(r % 6)) for r in range(60)])
    base = RW.select_rows(w, (b"items",))
    nr, rows = ctx.select_rows((b"items",))
    before = fetched(ctx, nr, rows)
    for values, negate in (([b"v1", b"v8"], False), ([b"v1"], True), ([], False), ([], True)):
        want = IW.where_in(w, base, K, S, values, negate)
        assert ctx.count_where_path_in(K, S, values, negate) == len(want[1])
        same_selection(fetched(ctx, nr, rows), before, (values, negate))
    assert ctx.where_path_in(K, S, [b"v1", b"v8"]) == (nr, ctx.count_where_path_in(K, S, [b"v1", b"v8", b"v3"]))  # (the count runs on the kept rows)
    ctx.select_records()


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_touch_nothing(ctx):
    import sjhip
    nd(ctx, ['{"k":"v%d","n":%d}' % (r % 4, r) for r in range(20)])
    assert ctx.where_path_in(K, S, [b"v1", b"v2"]) == (20, 10)
    before = fetched(ctx, 20, 10)
    L, h = sjhip.lib(), ctx._h
    u64 = lambda *x: np.array(x, dtype=np.uint64)  # noqa: E731
    data = np.frombuffer(b"abcdef" + b"x" * 1100, dtype=np.uint8)
    klen, nr, nw, cnt = (C.c_uint32 * 1)(1), C.c_size_t(77), C.c_size_t(77), C.c_uint64(77)
    cases = [  # (kind, offsets, values, n_values, flags, what the message names)
        (ctx.COL_FLOAT, None, u64(1), 1, 0, "kind 0"), (ctx.COL_BOOL, None, u64(1), 1, 0, "kind 3"), (ctx.COL_STRING_CVT, u64(0, 1), data, 1, 0, "kind 5"),
        (17, None, u64(1), 1, 0, "kind 17"), (-1, None, u64(1), 1, 0, "kind -1"),
        (I, None, u64(1), 1, 2, "flag bits 0x2"), (S, u64(0, 1), data, 1, 0x80000001, "flag bits 0x80000000"),
        (I, None, u64(1), (1 << 24) + 1, 0, "16777217 values"), (S, u64(0, 1), data, (1 << 24) + 1, 0, "16777217 values"),
        (I, None, None, 2, 0, "`values` is null"), (S, u64(0, 3), None, 1, 0, "`values` is null"), (S, None, data, 2, 0, "`value_offsets` is null"),
        (S, u64(1, 3, 5), data, 2, 0, "value_offsets[0]"), (S, u64(0, 3, 2, 6), data, 3, 0, "value_offsets[2]"),
        (S, u64(0, 3, 3, 1028, 1030), data, 4, 0, "value 2 is 1025 bytes"),
    ]
    for kind, offs, values, n, flags, names in cases:
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        for rc in (L.sjhip_where_path_in(h, b"k", klen, 1, kind, ptr(offs), ptr(values), n, flags, C.byref(nr), C.byref(nw)),
                   L.sjhip_count_where_path_in(h, b"k", klen, 1, kind, ptr(offs), ptr(values), n, flags, C.byref(cnt))):
            assert rc == 5 and names in ctx.last_error(), (names, ctx.last_error())
            same_selection(fetched(ctx, 20, 10), before, names)
    assert (nr.value, nw.value, cnt.value) == (77, 77, 77)
    for path in ((b"k",) * 17, (b"k" * 600, b"j" * 600)):  # a bad path
        for call in (ctx.where_path_in, ctx.count_where_path_in):
            with pytest.raises(sjhip.ParseError) as e:
                call(path, S, [b"v1"])
            assert e.value.code == 5
            same_selection(fetched(ctx, 20, 10), before, "path")
    assert L.sjhip_where_path_in(h, b"k", klen, 1, I, None, None, 0, 0, None, C.byref(nw)) == 5
    # a value of exactly 1024 bytes, equal offsets (empty values) and no values with null pointers are legal
    assert L.sjhip_count_where_path_in(h, b"k", klen, 1, S, ptr(u64(0, 0, 1024, 1024)), ptr(data), 3, 0, C.byref(cnt)) == 0 and cnt.value == 0
    assert L.sjhip_count_where_path_in(h, b"k", klen, 1, S, None, None, 0, 1, C.byref(cnt)) == 0 and cnt.value == 10
    same_selection(fetched(ctx, 20, 10), before, "legal calls")
    ctx.select_records()
    # no result on the device
    fresh = sjhip.Context(0)
    with pytest.raises(sjhip.ParseError) as e:
        fresh.where_path_in(K, I, [1])
    assert e.value.code == 5
    assert fresh.device_bytes() == 0
    fresh.parse(b'{"k":1}\n{"k":2}', ndjson=True)
    assert fresh.count_where_path(K, fresh.OP_EQ_INT, 2) == 1  # (the count's work arena is there now)
    base = fresh.device_bytes()
    assert fresh.count_where_path_in(K, I, [2, 3]) == 1 and fresh.device_bytes() > base  # the set's arena is counted
    assert fresh.where_path_in(K, I, [2, 3]) == (2, 1)
    fresh.trim()
    assert fresh.device_bytes() == 0  # the set's arena went with the others
    fresh.close()


@pytest.mark.parametrize("name", ["ABC", "BAB"])
def test_sharded_result_equals_whole(name):
    import test_gpu_product_parts as PP
    one, many = PP.contexts(name)
    try:
        ids = one.extract_path((b"id",), one.COL_INT)[0]
        got = []
        for c in (one, many):
            c.select_records()
            count = c.count_where_path_in((b"id",), I, ids[::3])
            nr, rows = c.where_path_in((b"id",), I, ids[::3])
            assert count == rows > 0
            sel = fetched(c, nr, rows)
            nr2, rows2 = c.where_path_in((b"id",), I, ids[::6], negate=True)
            got.append((nr, rows, sel, nr2, rows2, fetched(c, nr2, rows2)))
        a, b = got
        assert a[:2] == b[:2] and a[3:5] == b[3:5] and 0 < a[4] < a[1] < a[0]
        PP.same(b[2], a[2], (name, "rows"))
        PP.same(b[5], a[5], (name, "rows, narrowed twice"))
    finally:
        one.select_records()
        many.select_records()
