"""GPU: the grouping (sjhip_group_path / sjhip_fetch_groups / sjhip_fetch_group_aggregates) against the serial restatement of
tests/group_walk.py over the oracle's parse: on row counts around the wave and the largest tile of the new kernels (T =
GROUP_SORT_TILE rows), with one group, with every row its own group and with two alternating keys; on more groups than one and than
two sort digits cover; on keys that differ late, that are prefixes of each other, that are empty, that are long, and that are
spelled with and without an escape; on every key status; on INT keys; on the three value kinds, sums beyond 64 bits and the order
of the zeros; under a selection and a row predicate; and through the lifecycle and the error paths.

codes, status, keys, first_row, group_rows, counts, integer sums, min and max are compared exactly.  A float sum is compared as bits
where every partial sum of the values is exact (small integers and quarters), and otherwise against math.fsum within
(n - 1) u / (1 - (n - 1) u) * sum |x|, u = 2^-53, the bound tests/test_gpu_aggregate.py uses: it holds for every association."""
import ctypes as C
import random

import numpy as np
import pytest

import aggregate_walk as AW
import column_walk as CW
import fixtures
import group_walk as GW
import query_walk as Q
import rows_walk as RW
import where_walk as WW
from test_group_walk import STATUS_DOC
from test_gpu_aggregate import bits, check_aggregates, float_bound
from test_gpu_columns import oracle_walk
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

F, I, U, S = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT, GW.COL_STRING
T = GW.GROUP_SORT_TILE
NONE = GW.GROUP_NONE
ERR_ARG = 5
NAMES = ("count", "not_ok", "sum", "sum_hi", "min", "max")


def check_group(ctx, rw, key_path, key_kind, value_path=None, value_kind=None, exact=True, what=None):
    """group_path on the selection in force equals the checker; rw: a walk whose records() are the rows of that selection"""
    what = (what, key_path, key_kind, value_path, value_kind)
    want = GW.group(rw, key_path, key_kind, value_path, value_kind)
    got = ctx.group_path(key_path, key_kind, value_path, value_kind)
    print(what, "rows:", got.rows, "groups:", got.groups, "key bytes:", got.key_bytes, "want groups:", want.groups)
    assert (got.rows, got.groups) == (want.rows, want.groups), what
    assert got.status.dtype == np.uint8 and got.status.tolist() == want.status, what
    assert got.codes.dtype == np.uint32 and np.array_equal(got.codes, np.array(want.codes, dtype=np.uint32)), what
    if key_kind == S:
        assert got.keys == want.keys and got.key_bytes == sum(map(len, want.keys)), what
        assert int(got.key_offsets[0]) == 0 and int(got.key_offsets[-1]) == got.key_bytes, what
    else:
        assert got.keys.dtype == np.int64 and got.keys.tolist() == want.keys and got.key_bytes == 8 * want.groups, what
    assert got.first_row.tolist() == want.first_row and got.group_rows.tolist() == want.group_rows, what
    if value_kind is None:
        assert not hasattr(got, "count")
        return got, want
    dt = {F: np.float64, I: np.int64, U: np.uint64}[value_kind]
    arrays = got.aggregates()
    assert [a.dtype for a in arrays] == [np.uint64, np.uint64, dt, np.uint64, dt, dt], what
    wanted = GW.arrays(want, value_kind)
    for j, name in enumerate(NAMES):
        assert len(arrays[j]) == want.groups, (what, name)
        if name == "sum" and value_kind == F and not exact:
            vals, vsts = AW.column(rw, () if value_path is None else value_path, F)
            members = [[] for _ in range(want.groups)]
            for r, c in enumerate(want.codes):
                if c != NONE:
                    members[c].append(r)
            for g, rows in enumerate(members):
                bound = float_bound([vals[r] for r in rows], [vsts[r] for r in rows])
                if bound:
                    print(what, "group", g, "sum:", float(arrays[j][g]), "fsum:", want.aggs[g].sum, "bound:", bound)
                assert abs(float(arrays[j][g]) - want.aggs[g].sum) <= bound, (what, g)
            continue
        bad = np.flatnonzero(bits(arrays[j]) != np.array(wanted[j], dtype=np.uint64))
        assert len(bad) == 0, (what, name, bad[:5], bits(arrays[j])[bad[:5]], [wanted[j][k] for k in bad[:5]])
    assert int(got.group_rows.sum()) == want.status.count(CW.COL_OK), what
    assert np.array_equal(arrays[0] + arrays[1], got.group_rows), what
    return got, want


def nd_rows(ctx, lines):
    """the lines as an ND document without a selection: the rows are the records"""
    doc = "\n".join(lines).encode()
    ctx.parse(doc, ndjson=True)
    return oracle_walk(doc, True, True)


def array_rows(ctx, rows, copy=True):
    """{"rows":[...]} with the selection on "rows\""""
    doc = ('{"rows":[%s]}' % ",".join(rows)).encode()
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy)
    offs, index, sts = RW.select_rows(w, (b"rows",))
    assert ctx.select_rows((b"rows",)) == (1, len(index)) and len(index) == len(rows)
    return RW.RowWalk(w, index)


# ---- 1. shapes: the wave, the tile, and the three key patterns -----------------------------------------------------------------------
PATTERNS = {"one-group": lambda r: "same", "all-distinct": lambda r: "k%d" % r, "two-alternating": lambda r: "ab"[r % 2]}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_shapes(ctx, n, pattern):
    key = PATTERNS[pattern]
    # small integers of both signs: every float sum is exact in any association; every 11th row has no OK value
    lines = ['{"k":"%s","v":%s}' % (key(r), '"x"' if r % 11 == 10 else str((r + 1) * (-1 if r % 3 == 2 else 1))) for r in range(n)]
    w = nd_rows(ctx, lines)
    for kind in (F, I, U):
        got, want = check_group(ctx, w, (b"k",), S, (b"v",), kind, what=(pattern, n))
        assert got.groups == {"one-group": 1, "all-distinct": n, "two-alternating": min(n, 2)}[pattern]
    if pattern == "two-alternating" and n > 1:  # the order inside a group is the row order: its first row leads
        assert got.first_row.tolist() == [0, 1] and got.group_rows.tolist() == [(n + 1) // 2, n // 2]


def test_more_groups_than_one_digit(ctx):
    """700 rows over 300 keys cycling: two sort passes"""
    lines = ['{"k":"key-%d","v":%d.25}' % (r % 300, r) for r in range(700)]
    w = nd_rows(ctx, lines)
    got, want = check_group(ctx, w, (b"k",), S, (b"v",), F, what="300 keys")
    assert got.groups == 300 > 1 << GW.GROUP_RADIX_BITS and got.group_rows.tolist() == [3] * 100 + [2] * 200
    assert got.first_row.tolist() == list(range(300))


def big_lines():
    rnd = random.Random(19)
    lines, seen = [], []
    for r in range(70000):
        if rnd.random() < 2 / 3 or not seen:
            seen.append("u%x" % (r * 2654435761 & 0xFFFFFF | r << 24))
            k = seen[-1]
        else:
            k = seen[rnd.randrange(len(seen))] if rnd.random() < 0.5 else "hot%d" % rnd.randrange(5)
        lines.append('{"k":"%s","v":%d}' % (k, rnd.randrange(-1000, 1000)))
    return lines


def test_seventy_thousand_rows(ctx):
    """about two thirds of the rows distinct: real probing chains, a table of 2^18 slots filled to a sixth"""
    lines = big_lines()
    assert 1.2e6 < sum(map(len, lines)) < 2.2e6
    w = nd_rows(ctx, lines)
    got, want = check_group(ctx, w, (b"k",), S, (b"v",), I, what="70000")
    assert 44000 < got.groups < 49000 and got.rows == 70000
    assert int(got.group_rows.max()) > 1000  # the five hot keys


def test_more_groups_than_two_digits(ctx):
    """66 000 distinct INT keys and a few repeats: three sort passes (2^16 < groups)"""
    n = 66000
    lines = ['{"k":%d}' % (r * 7919 - 250000000 if r % 1000 else 42) for r in range(n)]
    w = nd_rows(ctx, lines)
    got, want = check_group(ctx, w, (b"k",), I, (), None, what="66000")
    assert got.groups == n - 65 > 1 << (2 * GW.GROUP_RADIX_BITS) and int(got.group_rows[0]) == 66
    got, want = check_group(ctx, w, (), S, (b"k",), I, what="66000 rows without a key")  # objects are no strings: no group
    assert got.groups == 0 and set(got.codes.tolist()) == {NONE}


# ---- 2. key equality ---------------------------------------------------------------------------------------------------------------
LONG = "".join(chr(97 + (i * 7) % 26) for i in range(4999))
KEY_CASES = {
    "last-byte": ["abcdefgh1", "abcdefgh2", "abcdefgh1", "abcdefg", "abcdefg1", "abcdefgh2", "abcdefghijklmnop", "abcdefghijklmnoq", "abcdefghijklmnop"],
    "prefix": ["ab", "abc", "a", "ab", "abcd", "abc", "abcdefghi", "abcdefgh", "abcdefghi"],
    "empty": ["", "a", "", " ", "", "a"],
    "long": [LONG + "x", LONG + "x", LONG + "y", "short", LONG + "x", LONG + "y", LONG],
}


@pytest.mark.parametrize("case", sorted(KEY_CASES))
def test_key_equality(ctx, case):
    keys = KEY_CASES[case]
    rw = array_rows(ctx, ['{"k":"%s","v":%d}' % (k, r + 1) for r, k in enumerate(keys)])
    got, want = check_group(ctx, rw, (b"k",), S, (b"v",), U, what=case)
    order = list(dict.fromkeys(keys))
    assert got.keys == [k.encode() for k in order] and got.codes.tolist() == [order.index(k) for k in keys]
    if case == "long":
        assert got.group_rows.tolist() == [3, 2, 1, 1] and len(got.keys[0]) == 5000


@pytest.mark.parametrize("copy", [True, False], ids=["copied", "in-the-message"])
def test_escaped_spelling_is_the_same_key(ctx, copy):
    """without copied strings "A" lies in the message and its escaped spelling in Strings.B"""
    rows = ['{"k":"A"}', '{"k":"\\u0041"}', '{"k":"B"}', '{"k":"\\u0041\\u0042"}', '{"k":"AB"}', '{"k":"\\u0042"}', '{"k":"a\\nb"}', '{"k":"a\\u000ab"}']
    rw = array_rows(ctx, rows, copy=copy)
    got, want = check_group(ctx, rw, (b"k",), S, what=("escaped", copy))
    assert got.keys == [b"A", b"B", b"AB", b"a\nb"] and got.codes.tolist() == [0, 0, 1, 2, 2, 1, 3, 3]
    ctx.select_records()


# ---- 3. statuses, INT keys -----------------------------------------------------------------------------------------------------------
def status_rows(ctx):
    w = oracle_walk(STATUS_DOC, False, True)
    ctx.parse(STATUS_DOC)
    offs, index, sts = RW.select_rows(w, (b"rows",))
    ctx.select_rows((b"rows",))
    return RW.RowWalk(w, index)


def test_every_key_status(ctx):
    rw = status_rows(ctx)
    got, want = check_group(ctx, rw, (b"k",), S, (b"v",), F, what="statuses")
    assert got.keys == [b"b", b"a", b""] and sorted(set(got.status.tolist())) == [0, 1, 2, 3, 4]
    assert got.codes.tolist() == [0, NONE, NONE, 1, NONE, NONE, 0, NONE, NONE, 2, 1, NONE, 0]
    assert (got.count.tolist(), got.not_ok.tolist(), got.sum.tolist()) == ([1, 2, 1], [2, 0, 0], [1.0, 6.5, -3.0])
    got, want = check_group(ctx, rw, (b"k",), I, (b"v",), I, what="statuses, INT keys")
    assert got.keys.tolist() == [12] and sorted(set(got.status.tolist())) == [0, 1, 2, 3, 4, 5] and got.sum.tolist() == [8]
    got, want = check_group(ctx, rw, (b"nope",), S, (b"v",), F, what="no OK key")
    assert got.groups == 0 and got.key_bytes == 0 and got.key_offsets.tolist() == [0] and len(got.sum) == 0
    assert set(got.codes.tolist()) == {NONE} and set(got.status.tolist()) == {CW.COL_NOT_FOUND, CW.COL_NOT_OBJECT}
    ctx.select_records()


def test_int_keys(ctx):
    rows = ["1", "1.0", "1.9", "-1", "-1.5", "9223372036854775808.0", "18446744073709551615", "-9223372036854775808", "0", "-0.0", '"1"',
            "-7", "1e300", "null", "-7.99"]
    rw = array_rows(ctx, ['{"k":%s,"v":%d}' % (k, r) for r, k in enumerate(rows)])
    got, want = check_group(ctx, rw, (b"k",), I, (b"v",), I, what="int keys")
    assert got.keys.tolist() == [1, -1, -(1 << 63), 0, -7] and got.codes.tolist() == [0, 0, 0, 1, 1, 2, NONE, 2, 3, 3, NONE, 4, NONE, NONE, 4]
    assert got.status[6] == CW.COL_RANGE and got.status[12] == CW.COL_RANGE and got.status[13] == CW.COL_NULL
    ctx.select_records()


# ---- 4. the value column ---------------------------------------------------------------------------------------------------------------
def test_sums_beyond_64_bits(ctx):
    hi, lo, top = (1 << 63) - 1, -(1 << 63), (1 << 64) - 1
    vals = {"p": [hi] * 300, "m": [lo] * 40 + [hi] * 10, "t": [top] * 300}
    rows = [(k, vals[k][j]) for j in range(300) for k in "pmt" if j < len(vals[k])]  # interleaved: the sort brings the groups together
    rw = array_rows(ctx, ['{"k":"%s","v":%d}' % kv for kv in rows])
    got, want = check_group(ctx, rw, (b"k",), S, (b"v",), I, what="int sums")
    assert [a.sum for a in want.aggs] == [300 * hi, 40 * lo + 10 * hi, 0] and got.sum_hi.tolist()[0] == (300 * hi) >> 64 != 0
    assert got.not_ok.tolist() == [0, 0, 300]  # MaxUint64 is RANGE for INT
    got, want = check_group(ctx, rw, (b"k",), S, (b"v",), U, what="uint sums")
    assert [a.sum for a in want.aggs] == [300 * hi, 10 * hi, 300 * top] and got.sum_hi.tolist() == [(300 * hi) >> 64, (10 * hi) >> 64, 299]
    ctx.select_records()


def test_float_sums_bound_determinism_and_zeros(ctx):
    rnd = random.Random(20252)
    n = 2 * T + 77
    xs = [rnd.choice((-1.0, 1.0)) * 10.0 ** rnd.uniform(-3, 12) for _ in range(n)]
    rw = array_rows(ctx, ['{"k":"g%d","v":%r}' % (rnd.randrange(3), x) for x in xs] +
                    ['{"k":"z1","v":-0.0}', '{"k":"z1","v":0.0}', '{"k":"z2","v":0.0}', '{"k":"z2","v":-0.0}', '{"k":"z3","v":-0.0}', '{"k":"z3","v":-0.0}',
                     '{"k":"none","v":null}'])
    got, want = check_group(ctx, rw, (b"k",), S, (b"v",), F, exact=False, what="float")
    assert got.keys[-4:] == [b"z1", b"z2", b"z3", b"none"]
    neg0 = 1 << 63
    assert bits(got.min)[-4:].tolist() == [neg0, neg0, neg0, 0] and bits(got.max)[-4:].tolist() == [0, 0, neg0, 0]  # -0.0 below +0.0
    assert bits(got.sum)[-4:].tolist() == [0, 0, neg0, 0] and got.count.tolist()[-1] == 0 and got.not_ok.tolist()[-1] == 1
    again = ctx.group_path((b"k",), S, (b"v",), F)
    for a, b in zip(got.aggregates(), again.aggregates()):
        assert np.array_equal(bits(a), bits(b))  # the same bits from every call
    assert np.array_equal(got.codes, again.codes)
    ctx.select_records()


def test_no_value(ctx):
    import sjhip
    rw = array_rows(ctx, ['{"k":"a"}', '{"k":"b"}', '{"k":"a"}'])
    got, want = check_group(ctx, rw, (b"k",), S, what="no value")
    assert got.group_rows.tolist() == [2, 1]
    out = np.full(2, 7, dtype=np.uint64)
    assert sjhip.lib().sjhip_fetch_group_aggregates(ctx._h, out.ctypes.data, None, None, None, None, None) == ERR_ARG
    assert "no value column" in ctx.last_error() and out.tolist() == [7, 7]
    # the value path is ignored with SJHIP_GROUP_NO_VALUE, whatever it holds
    nr, ng, nb = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    lens = (C.c_uint32 * 1)(1)
    assert sjhip.lib().sjhip_group_path(ctx._h, b"k", lens, 1, S, None, None, 99, -1, C.byref(nr), C.byref(ng), C.byref(nb)) == 0
    assert (nr.value, ng.value, nb.value) == (3, 2, 2)
    ctx.select_records()


# ---- 5. under a selection ------------------------------------------------------------------------------------------------------------
def test_twitter_statuses(ctx):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    base = RW.select_rows(w, (b"statuses",))
    assert ctx.select_rows((b"statuses",)) == (1, len(base[1]))
    rw = RW.RowWalk(w, base[1])
    got, want = check_group(ctx, rw, (b"lang",), S, (b"retweet_count",), I, what="lang")
    assert dict(zip(got.keys, got.group_rows.tolist())) == {b"ja": 96, b"zh": 4}
    check_group(ctx, rw, (b"user", b"screen_name"), S, (b"retweet_count",), F, exact=False, what="screen_name")
    check_group(ctx, rw, (b"user", b"id"), I, (b"user", b"followers_count"), U, what="user.id")
    check_group(ctx, rw, (b"geo",), S, (b"retweet_count",), I, what="geo: null")
    # the same after a predicate; then one that keeps no row
    sel = WW.where(w, base, (b"lang",), Q.OP_EQ_STRING, b"zh")
    assert ctx.where_path((b"lang",), ctx.OP_EQ_STRING, b"zh") == (1, 4)
    kept = RW.RowWalk(w, sel[1])
    got, want = check_group(ctx, kept, (b"user", b"screen_name"), S, (b"retweet_count",), I, what="where zh")
    assert got.rows == 4
    assert ctx.where_path((b"lang",), ctx.OP_EQ_STRING, b"en") == (1, 0)
    got, want = check_group(ctx, RW.RowWalk(w, []), (b"lang",), S, (b"retweet_count",), I, what="no rows")
    assert (got.rows, got.groups, got.key_bytes) == (0, 0, 0) and got.key_offsets.tolist() == [0] and got.keys == [] and len(got.codes) == 0
    ctx.select_records()
    got, want = check_group(ctx, w, (b"search_metadata", b"query"), S, (b"search_metadata", b"count"), I, what="the record")
    assert (got.rows, got.groups) == (1, 1)


def test_empty_path_over_scalar_rows(ctx):
    doc = b'{"hashtags":["a","b","a",1,null,"b","a","\\u0061"],"n":[3,3.5,"3",4,4.0]}'
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    for path, kind, vkind in [((b"hashtags",), S, None), ((b"n",), I, U), ((b"n",), I, F)]:
        offs, index, sts = RW.select_rows(w, path)
        ctx.select_rows(path)
        got, want = check_group(ctx, RW.RowWalk(w, index), (), kind, (), vkind, what=path)
    assert got.keys.tolist() == [3, 4] and got.sum.tolist() == [6.5, 8.0]
    ctx.select_records()


# ---- 6. lifecycle, errors --------------------------------------------------------------------------------------------------------------
def same_groups(a, b):
    assert (a.rows, a.groups, a.keys if isinstance(a.keys, list) else a.keys.tolist()) == (b.rows, b.groups, b.keys if isinstance(b.keys, list) else b.keys.tolist())
    for x, y in zip((a.first_row, a.group_rows, a.codes, a.status) + a.aggregates(), (b.first_row, b.group_rows, b.codes, b.status) + b.aggregates()):
        assert np.array_equal(bits(x) if x.dtype.itemsize == 8 else x, bits(y) if y.dtype.itemsize == 8 else y)


def test_lifecycle(ctx):
    import sjhip
    L = sjhip.lib()
    doc = fixtures.load("twitter")
    ctx.trim()
    ctx.parse(doc, key_flags=True)
    ctx.select_rows((b"statuses",))
    before = ctx.device_bytes()
    first = ctx.group_path((b"user", b"screen_name"), S, (b"retweet_count",), I)
    assert ctx.device_bytes() > before  # the arena of the grouping is counted
    sizes = ctx.group_path((b"user", b"screen_name"), S, (b"retweet_count",), I, fetch=False)
    # it survives the drop and the change of the selection, a string column, a table, a list column, MarshalJSON ...
    ctx.select_records()
    ctx.extract_path_strings((b"search_metadata", b"query"))
    ctx.extract_table([((b"search_metadata", b"count"), I), ((b"search_metadata", b"query"), S)])
    text = ctx.marshal_json()
    ctx.select_rows((b"statuses",))
    ctx.where_path((b"lang",), ctx.OP_EQ_STRING, b"zh")
    same_groups(ctx.fetch_groups(sizes), first)
    # ... and they survive it: the selection, the column and the text are as they were
    off, idx, st = ctx.fetch_rows(1, 4)
    assert off.tolist() == [0, 4]
    assert ctx.marshal_json() == text
    # a second call replaces it
    second = ctx.group_path((b"lang",), S)
    assert second.keys == [b"zh"] and second.rows == 4
    assert L.sjhip_fetch_group_aggregates(ctx._h, None, None, None, None, None, None) == ERR_ARG and "no value column" in ctx.last_error()
    # bad kinds and bad paths touch nothing: the grouping, the selection and the other products stay fetchable and unchanged
    nr, ng, nb = C.c_size_t(77), C.c_size_t(77), C.c_size_t(77)
    lens = (C.c_uint32 * 1)(4)
    sizes3 = (C.byref(nr), C.byref(ng), C.byref(nb))
    for kk, vk, word in [(F, -1, "key kind 0"), (U, -1, "key kind 2"), (5, -1, "key kind 5"), (99, I, "key kind 99"), (S, 3, "value kind 3"),
                         (S, 4, "value kind 4"), (I, -2, "value kind -2")]:
        assert L.sjhip_group_path(ctx._h, b"lang", lens, 1, kk, b"lang", lens, 1, vk, *sizes3) == ERR_ARG
        assert word in ctx.last_error() and (nr.value, ng.value, nb.value) == (77, 77, 77), ctx.last_error()
    with pytest.raises(sjhip.ParseError):
        ctx.group_path((b"k",) * 17, S)  # a path longer than sjhip_find_path takes
    with pytest.raises(sjhip.ParseError):
        ctx.group_path((b"lang",), S, (b"k",) * 17, I)
    assert L.sjhip_group_path(ctx._h, None, None, 1, S, None, None, 0, -1, *sizes3) == ERR_ARG  # keys announced, none given
    assert L.sjhip_group_path(ctx._h, b"lang", lens, 1, S, None, None, 0, -1, None, None, None) == ERR_ARG
    same_groups_keys = ctx.fetch_groups(sjhip.Groups(second.rows, second.groups, second.key_bytes, S, None))
    assert same_groups_keys.keys == [b"zh"] and same_groups_keys.codes.tolist() == [0] * 4
    assert ctx.fetch_rows(1, 4)[1].tolist() == idx.tolist()
    ctx.select_records()
    # a parse drops it; so does a trim, which frees its arena
    ctx.parse(b'{"a":1}')
    assert L.sjhip_fetch_groups(ctx._h, None, None, None, None, None, None) == ERR_ARG and "no grouping" in ctx.last_error()
    assert L.sjhip_fetch_group_aggregates(ctx._h, None, None, None, None, None, None) == ERR_ARG and "no grouping" in ctx.last_error()
    g = ctx.group_path((b"a",), I, (b"a",), I)
    assert g.keys.tolist() == [1] and g.sum.tolist() == [1]
    assert L.sjhip_fetch_groups(ctx._h, None, None, None, None, None, None) == 0  # every destination null
    ctx.trim()
    assert ctx.device_bytes() == 0
    assert L.sjhip_fetch_groups(ctx._h, None, None, None, None, None, None) == ERR_ARG
    fresh = sjhip.Context(0)  # no result on the device
    assert L.sjhip_group_path(fresh._h, b"lang", lens, 1, S, None, None, 0, -1, *sizes3) == ERR_ARG and fresh.last_error()
    assert L.sjhip_fetch_groups(fresh._h, None, None, None, None, None, None) == ERR_ARG
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
            many.group_path((b"k",), S)
        assert "sharded" in many.last_error()
        assert many.aggregate_path((b"k",), I).status[CW.COL_TYPE] == 11000  # the result is as it was
    finally:
        many.close()


def test_aggregates_after_all_of_it(ctx):
    """the existing aggregate calls, whose kernel took the grouping's row permutation, after group calls in the same context"""
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    offs, index, sts = RW.select_rows(w, (b"statuses",))
    ctx.select_rows((b"statuses",))
    rw = RW.RowWalk(w, index)
    check_group(ctx, rw, (b"user", b"screen_name"), S, (b"retweet_count",), I, what="before the aggregates")
    for path in [(b"retweet_count",), (b"user", b"followers_count")]:
        for kind in (F, I, U):
            check_aggregates(ctx, rw, offs, path, kind, exact=False, what="after a grouping")
    ctx.select_records()
