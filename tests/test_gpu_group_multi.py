"""GPU: the grouping by several keys (sjhip_group_paths / sjhip_fetch_group_keys / sjhip_fetch_group_aggregates_at) against the
serial restatement of tests/group_multi_walk.py over the oracle's parse: on row counts around the wave, the block, the tile and the
capacity step of the table, with one group, all tuples distinct and 17 x 17 values; on tuple equality (column boundaries, swapped
entries, kinds, 8 columns that differ in one, key lengths around the word and the lane / wave copy switch, the empty string against
"no key", escaped spellings in both copy modes); on the colliding and slot-homed families of tests/group_multi_table.py; on every
status with and without SJHIP_GROUP_NULL_KEY; on UINT, BOOL and INT keys, an empty path and a composed selection; on 0, 1, 2 and 8
value columns against the single-value grouping, bit for bit; on identity with sjhip_group_path through both families of fetches;
and through the errors and the lifecycle.  Everything is compared exactly: the float values are exactly representable (small
integers and quarters), so every association of their sums gives the same bits."""
import ctypes as C

import numpy as np
import pytest

import column_walk as CW
import fixtures
import group_multi_table as MT
import group_multi_walk as MW
import group_walk as GW
import query_walk as Q
import rows_walk as RW
import where_walk as WW
from test_group_walk import STATUS_DOC
from test_gpu_aggregate import bits
from test_gpu_columns import oracle_walk
from test_gpu_group import array_rows, nd_rows
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

F, I, U, B, S = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT, CW.COL_BOOL, GW.COL_STRING
T = GW.GROUP_SORT_TILE
NONE = MW.GROUP_NONE
ERR_ARG = 5
DT = {F: np.float64, I: np.int64, U: np.uint64}


def check(ctx, rw, key_columns, value_columns=(), what=None):
    """group_paths on the selection in force equals the checker; rw: a walk whose records() are the rows of that selection"""
    want = MW.group(rw, key_columns, value_columns)
    got = ctx.group_paths(key_columns, value_columns)
    kinds = [c[1] for c in key_columns]
    print(what, key_columns, "rows:", got.rows, "groups:", got.groups, "key bytes:", got.key_bytes, "want groups:", want.groups)
    assert (got.rows, got.groups) == (want.rows, want.groups), what
    assert got.key_bytes == MW.key_bytes(want, kinds), what
    assert got.codes.dtype == np.uint32 and np.array_equal(got.codes, np.array(want.codes, dtype=np.uint32)), what
    assert got.first_row.tolist() == want.first_row and got.group_rows.tolist() == want.group_rows, what
    for c, kind in enumerate(kinds):
        assert got.status[c].dtype == np.uint8 and got.status[c].tolist() == want.status[c], (what, c)
        assert got.key_ok[c].dtype == np.uint8 and got.key_ok[c].tolist() == want.key_ok[c], (what, c)
        if kind == S:
            assert got.keys[c] == [b"" if k is None else k for k in want.keys[c]], (what, c)
            assert int(got.key_offsets[c][0]) == 0 and int(got.key_offsets[c][-1]) == got.key_bytes[c], (what, c)
        else:
            assert got.keys[c].dtype == {I: np.int64, U: np.uint64, B: np.uint8}[kind], (what, c)
            assert got.keys[c].tolist() == [0 if k is None else k for k in want.keys[c]], (what, c)
    assert len(got.values) == len(value_columns)
    for v, (_, kind) in enumerate(value_columns):
        arrays, wanted = got.values[v], MW.arrays(want, v, kind)
        assert [a.dtype for a in arrays] == [np.uint64, np.uint64, DT[kind], np.uint64, DT[kind], DT[kind]], (what, v)
        for j in range(6):
            assert np.array_equal(bits(arrays[j]), np.array(wanted[j], dtype=np.uint64)), (what, v, j)
        assert np.array_equal(arrays[0] + arrays[1], got.group_rows), (what, v)
    return got, want


# ---- 1. shapes -----------------------------------------------------------------------------------------------------------------------
PATTERNS = {"one-group": lambda r: ("same", 7), "all-distinct": lambda r: ("k%d" % (r % 5), r), "17x17": lambda r: ("m%d" % (r % 17), r // 17 % 17)}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n", [1, 32, 33, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_shapes(ctx, n, pattern):
    key = PATTERNS[pattern]
    lines = ['{"a":"%s","b":%d,"v":%s}' % (key(r) + ('"x"' if r % 11 == 10 else str((r + 1) * (-1 if r % 3 == 2 else 1)),)) for r in range(n)]
    w = nd_rows(ctx, lines)
    got, _ = check(ctx, w, [((b"a",), S), ((b"b",), I)], [((b"v",), F), ((b"v",), I)], what=(pattern, n))
    assert got.groups == {"one-group": 1, "all-distinct": n, "17x17": min(n, 289)}[pattern]


# ---- 2. tuple equality ---------------------------------------------------------------------------------------------------------------
def test_column_boundaries_swaps_and_kinds(ctx):
    rows = ['{"a":"ab","b":"c"}', '{"a":"a","b":"bc"}', '{"a":"c","b":"ab"}', '{"a":"ab","b":"c"}', '{"a":"","b":"abc"}', '{"a":"abc","b":""}',
            '{"a":"1","b":1}', '{"a":1,"b":"1"}', '{"a":"1","b":1.0}']
    rw = array_rows(ctx, rows)
    got, _ = check(ctx, rw, [((b"a",), S), ((b"b",), S)], what="boundaries")
    assert got.codes.tolist() == [0, 1, 2, 0, 3, 4, NONE, NONE, NONE]
    check(ctx, rw, [((b"a",), S, True), ((b"b",), S, True)], what="boundaries, flags")
    # INT 1 against STRING "1" in the same position of different calls
    a, _ = check(ctx, rw, [((b"a",), S, True), ((b"b",), I, True)], what="string, int")
    b, _ = check(ctx, rw, [((b"a",), I, True), ((b"b",), S, True)], what="int, string")
    assert a.codes[6] == a.codes[8] != a.codes[7] and b.codes[6] != b.codes[7]


def test_eight_columns_that_differ_in_one(ctx):
    fam = MT.families()["all_but_one"]
    rw = array_rows(ctx, MT.rows_json(fam))
    got, _ = check(ctx, rw, MT.key_columns(fam, S, I), [((b"v",), I)], what="all but one")
    assert got.groups == 9 and got.codes.tolist() == list(range(9)) + list(range(8, -1, -1))


@pytest.mark.parametrize("copy", [True, False], ids=["copied", "in-message"])
def test_key_lengths_empty_against_no_key_and_escapes(ctx, copy):
    rows = []
    for n in (0, 7, 8, 9, 31, 32, 33, 5000):
        key = ("k%d-" % n + "x" * n)[:n]
        twin = key[:-1] + "y" if n else ""
        rows += ['{"a":1,"b":"%s"}' % key, '{"a":1,"b":"%s"}' % twin, '{"a":2,"b":"%s"}' % key]
    rows += ['{"a":1}', '{"a":1,"b":null}', '{"a":1,"b":""}', '{"a":1,"b":"A"}', '{"a":1,"b":"\\u0041"}', '{"a":1,"b":"\\u0041\\u0041"}',
             '{"a":1,"b":"AA"}', '{"a":1,"b":"tab\\there"}', '{"a":1,"b":"tab\\u0009here"}']
    rows = rows + rows[::-1]
    rw = array_rows(ctx, rows, copy)
    got, want = check(ctx, rw, [((b"a",), I), ((b"b",), S, True)], [((b"a",), U)], what=("lengths", copy))
    no_key = got.codes[rows.index('{"a":1}')]
    assert got.key_ok[1][no_key] == 0 and got.keys[1][no_key] == b"" and no_key != got.codes[rows.index('{"a":1,"b":""}')]
    assert got.codes[rows.index('{"a":1,"b":"A"}')] == got.codes[rows.index('{"a":1,"b":"\\u0041"}')]
    assert max(map(len, got.keys[1])) == 5000


# ---- 3. the table on its seams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in MT.families() if n != "all_but_one"))
def test_table_families(ctx, name):
    fam = MT.families()[name]
    fam.check()
    rw = array_rows(ctx, MT.rows_json(fam))
    got, want = check(ctx, rw, MT.key_columns(fam, S, I), [((b"v",), I), ((b"v",), F)], what=fam.says)
    assert got.groups == len(set(fam.keys)) and sorted(got.first_row.tolist()) == got.first_row.tolist()


# ---- 4. every status on every column -------------------------------------------------------------------------------------------------
def test_every_status_on_column_1(ctx):
    doc = STATUS_DOC.replace(b'{"', b'{"j":1,"')
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    ctx.select_rows((b"rows",))
    rw = RW.on_rows(w, (b"rows",))
    for kind in (S, I, U):  # (INT and UINT: RANGE on the uint64 / the negative key)
        plain, _ = check(ctx, rw, [((b"j",), I), ((b"k",), kind)], [((b"v",), F)], what=("plain", kind))
        assert plain.status[0].tolist() == [0, 0, 2] + [0] * 10 and set(plain.codes[plain.status[1] != 0].tolist()) == {NONE}
        flagged, _ = check(ctx, rw, [((b"j",), I), ((b"k",), kind, True)], [((b"v",), F)], what=("flag on 1", kind))
        g = flagged.codes[1]
        assert flagged.key_ok[1][g] == 0 and set(flagged.codes[(flagged.status[1] != 0) & (flagged.status[0] == 0)].tolist()) == {g}
        assert flagged.codes[2] == NONE and flagged.first_row.tolist() == sorted(flagged.first_row.tolist())
        both, _ = check(ctx, rw, [((b"j",), I, True), ((b"k",), kind, True)], what=("both flags", kind))
        assert NONE not in both.codes.tolist() and both.key_ok[0][both.codes[2]] == 0 == both.key_ok[1][both.codes[2]]
    assert {1, 2, 3, 4, 5} <= set(check(ctx, rw, [((b"j",), I), ((b"k",), I, True)])[0].status[1].tolist())


# ---- 5. kinds, the empty path, a composed selection ----------------------------------------------------------------------------------
def test_uint_bool_and_int_keys(ctx):
    rows = ['{"u":18446744073709551615,"b":true,"i":1}', '{"u":18446744073709551615,"b":false,"i":1.0}', '{"u":9223372036854775808,"b":true,"i":1.9}',
            '{"u":18446744073709551615,"b":true,"i":2}', '{"u":-1,"b":true,"i":1}', '{"u":1,"b":1,"i":1}', '{"u":18446744073709551615,"b":true,"i":1.5}']
    rw = array_rows(ctx, rows)
    got, _ = check(ctx, rw, [((b"u",), U), ((b"b",), B), ((b"i",), I)], [((b"u",), U)], what="kinds")
    assert got.codes.tolist() == [0, 1, 2, 3, NONE, NONE, 0] and got.keys[0][0] == (1 << 64) - 1 and got.key_bytes == [32, 4, 32]
    assert int(got.values[0][3][0]) == 1 and int(got.values[0][2][0]) == (2 * ((1 << 64) - 1)) & ((1 << 64) - 1)  # a 128-bit sum
    check(ctx, rw, [((b"b",), B, True)], what="bool alone")


def test_empty_path_over_scalar_rows(ctx):
    doc = b'{"hashtags":["a","b","a",1,null,"b","a"],"n":[3,3.5,"3",4]}'
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    for path, cols in (((b"hashtags",), [((), S), ((), S, True)]), ((b"n",), [((), I, True), ((), U)])):
        ctx.select_rows(path)
        check(ctx, RW.on_rows(w, path), cols, [((), F)] if path == (b"n",) else [], what=path)


def test_after_select_where_and_unnest(ctx):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    base = RW.select_rows(w, (b"statuses",))
    assert ctx.select_rows((b"statuses",)) == (1, len(base[1]))
    rw = RW.RowWalk(w, base[1])
    # real data: statuses by (lang, user.verified) with sum(retweet_count) and max(favorite_count)
    got, _ = check(ctx, rw, [((b"lang",), S), ((b"user", b"verified"), B)], [((b"retweet_count",), I), ((b"favorite_count",), U)], what="twitter")
    assert got.groups > 1
    # hashtags per (text, indices: an array, so "no key") of the statuses in Japanese, after a predicate and an unnest
    sel = WW.where(w, base, (b"lang",), Q.OP_EQ_STRING, b"ja")
    assert ctx.where_path((b"lang",), ctx.OP_EQ_STRING, b"ja") == (1, len(sel[1]))
    import unnest_walk as UW
    un = UW.unnest_rows(RW.RowWalk(w, sel[1]), (b"entities", b"hashtags"), sel[0], sel[2])
    assert ctx.unnest_rows((b"entities", b"hashtags")) == (len(un[2]), len(un[5]), len(un[1])) and len(un[1]) > 1
    got, _ = check(ctx, RW.RowWalk(w, un[1]), [((b"text",), S), ((b"indices",), I, True)], what="hashtags")
    assert 1 < got.groups <= got.rows and set(got.key_ok[1].tolist()) == {0}


def test_sharded_result_is_refused(ctx):
    import sjhip
    pad = "x" * 230
    doc = "\n".join('{"pad":"%s","k":"%d"}' % (pad, r % 7) for r in range(11000)).encode()
    many = sjhip.Context(0)
    try:
        with fixtures.nd_shard_limits(2 << 20, 1 << 20):
            many.parse(doc, ndjson=True)
        with pytest.raises(sjhip.ParseError):
            many.group_paths([((b"k",), S), ((b"pad",), S)])
        assert "sharded" in many.last_error()
    finally:
        many.close()


# ---- 6. values -----------------------------------------------------------------------------------------------------------------------
def test_value_columns_equal_the_single_value_grouping(ctx):
    hi = (1 << 63) - 1
    lines = ['{"k":"%s","f":%d.25,"i":%d,"u":%d,"m":%s}' % ("abc"[r % 3], r - 40, hi if r % 2 else -(1 << 63), (1 << 64) - 1 - r, '"x"' if r % 5 == 0 else str(r))
             for r in range(1500)]
    w = nd_rows(ctx, lines)
    vals = [((b"f",), F), ((b"i",), I), ((b"u",), U), ((b"m",), F), ((b"m",), I), ((b"m",), U), ((b"none",), F), ((b"f",), I)]
    singles = [ctx.group_path((b"k",), S, path, kind).aggregates() for path, kind in vals]
    for n_vals in (0, 1, 2, 8):
        got, _ = check(ctx, w, [((b"k",), S)], vals[:n_vals], what=("values", n_vals))
        for v in range(n_vals):
            for j in range(6):
                assert np.array_equal(bits(got.values[v][j]), bits(singles[v][j])), (n_vals, v, j)


# ---- 7. identity with the single key's call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [S, I])
def test_one_column_is_group_path_through_both_fetch_families(ctx, kind):
    doc = STATUS_DOC
    ctx.parse(doc)
    ctx.select_rows((b"rows",))
    old = ctx.group_path((b"k",), kind, (b"v",), F)
    # the new fetches on a grouping group_path built: column 0 and value 0
    keys, off, key_ok, status = ctx.fetch_group_keys(0, kind, old.groups, old.key_bytes, old.rows)
    assert (keys == old.keys if kind == S else np.array_equal(keys, old.keys)) and key_ok.tolist() == [1] * old.groups
    assert np.array_equal(status, old.status)
    for a, b in zip(ctx.fetch_group_aggregates_at(0, F, old.groups), old.aggregates()):
        assert np.array_equal(bits(a), bits(b))
    L = ctx_lib()
    assert L.sjhip_fetch_group_keys(ctx._h, 1, None, None, None, None) == ERR_ARG and b"column 1" in ctx.last_error().encode()
    assert L.sjhip_fetch_group_aggregates_at(ctx._h, 1, None, None, None, None, None, None) == ERR_ARG
    new = ctx.group_paths([((b"k",), kind)], [((b"v",), F)])
    assert (new.rows, new.groups, new.key_bytes) == (old.rows, old.groups, [old.key_bytes])
    again = ctx.fetch_groups(type(old)(old.rows, old.groups, old.key_bytes, kind, F))  # the old fetches on the new grouping
    for name in ("first_row", "group_rows", "codes", "status", "count", "not_ok", "sum", "sum_hi", "min", "max"):
        assert getattr(again, name).dtype == getattr(old, name).dtype and getattr(again, name).tobytes() == getattr(old, name).tobytes(), name
        if name in ("first_row", "group_rows", "codes"):
            assert np.array_equal(getattr(new, name), getattr(old, name)), name
    assert (again.keys == old.keys) if kind == S else np.array_equal(again.keys, old.keys)
    assert (new.keys[0] == old.keys) if kind == S else np.array_equal(new.keys[0], old.keys)
    assert np.array_equal(new.status[0], old.status)
    for a, b in zip(new.values[0], old.aggregates()):
        assert np.array_equal(bits(a), bits(b))


def ctx_lib():
    import sjhip
    return sjhip.lib()


def test_old_fetches_are_refused_where_ambiguous(ctx):
    ctx.parse(STATUS_DOC)
    ctx.select_rows((b"rows",))
    L = ctx_lib()
    g = ctx.group_paths([((b"k",), S), ((b"v",), I, True)], [((b"v",), F), ((b"v",), I)], fetch=False)
    st, codes = np.empty(g.rows, dtype=np.uint8), np.empty(g.rows, dtype=np.uint32)
    assert L.sjhip_fetch_groups(ctx._h, None, None, None, None, None, st.ctypes.data) == ERR_ARG and "sjhip_fetch_group_keys" in ctx.last_error()
    assert L.sjhip_fetch_groups(ctx._h, None, None, None, None, codes.ctypes.data, None) == 0
    assert L.sjhip_fetch_group_aggregates(ctx._h, None, None, None, None, None, None) == ERR_ARG
    assert "sjhip_fetch_group_aggregates_at" in ctx.last_error()
    ctx.group_paths([((b"k",), S)], fetch=False)
    assert L.sjhip_fetch_group_aggregates(ctx._h, None, None, None, None, None, None) == ERR_ARG and "no value column" in ctx.last_error()
    assert L.sjhip_fetch_group_aggregates_at(ctx._h, 0, None, None, None, None, None, None) == ERR_ARG


# ---- 8. errors and lifecycle ---------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_previous_grouping(ctx):
    ctx.parse(STATUS_DOC)
    ctx.select_rows((b"rows",))
    before = ctx.group_paths([((b"k",), S), ((b"v",), I, True)], [((b"v",), F)])
    L = ctx_lib()
    one = [((b"k",), S)]
    import sjhip
    bad = [  # (key columns, value columns, fragments of the message)
        ([((b"k",), F)], [], ("key column 0", "kind 0")), ([((b"k",), S), ((b"k",), 5)], [], ("key column 1", "kind 5")),  # FLOAT, STRING_CVT
        ([((b"k",), 9)], [], ("key column 0", "kind 9")),
        (one, [((b"v",), S)], ("value column 0", "kind 4")), (one, [((b"v",), F), ((b"v",), B)], ("value column 1", "kind 3")),
        ([((b"k",), S)] * 9, [], ("9 key columns", "1 to 8")), ([], [], ("0 key columns", "1 to 8")),
        (one, [((b"v",), F)] * 9, ("9 value columns", "0 to 8")),
        ([((b"k",) * 5, S)] * 6 + [((b"k",) * 3, S)], [], ("more than 32 keys",)),                # 33 keys in paths of at most 5
        ([((b"k",) * 5, S)] * 6, [((b"k",) * 3, F)], ("more than 32 keys", "value column 0")),    # ... the 33rd in a value path
        ([((b"k" * 205,), S)] * 5, [], ("longer than 1024 bytes together",)),                     # 1025 bytes in paths of 205
    ]
    for kcols, vcols, fragments in bad:
        with pytest.raises(sjhip.ParseError) as e:
            ctx.group_paths(kcols, vcols)
        print(e.value)
        assert e.value.code == ERR_ARG and "sjhip_group_paths" in str(e.value) and all(f in str(e.value) for f in fragments), (fragments, e.value)
    nr, ng, nb = C.c_size_t(0), C.c_size_t(0), (C.c_size_t * 8)()
    pl, kinds, flags = (C.c_uint32 * 1)(1), (C.c_int * 1)(S), (C.c_uint32 * 1)(2)
    assert L.sjhip_group_paths(ctx._h, b"k", (C.c_uint32 * 1)(1), pl, kinds, flags, 1, None, None, 0, C.byref(nr), C.byref(ng), nb) == ERR_ARG
    assert "flag" in ctx.last_error()
    kinds[0] = F
    assert L.sjhip_group_paths(ctx._h, b"k", (C.c_uint32 * 1)(1), pl, kinds, None, 1, None, None, 0, C.byref(nr), C.byref(ng), nb) == ERR_ARG
    assert "column 0" in ctx.last_error() and "kind 0" in ctx.last_error()
    after = ctx.fetch_group_paths(type(before)(before.rows, before.groups, before.key_bytes, before.key_kind, before.value_kind))
    assert np.array_equal(after.codes, before.codes) and after.keys == before.keys[:1] + [after.keys[1]]
    assert np.array_equal(after.keys[1], before.keys[1]) and np.array_equal(bits(after.values[0][2]), bits(before.values[0][2]))


def test_no_rows_and_the_lifecycle(ctx):
    ctx.parse(b'{"rows":[]}')
    ctx.select_rows((b"rows",))
    g = ctx.group_paths([((b"k",), S), ((b"j",), I)], [((b"v",), F)])
    assert (g.rows, g.groups, g.key_bytes) == (0, 0, [0, 0]) and g.keys[0] == [] and len(g.keys[1]) == 0 and g.key_offsets[0].tolist() == [0]
    lines = ['{"k":"%s","j":%d,"v":%d}' % ("ab"[r % 2], r % 3, r) for r in range(100)]
    import sjhip
    ctx.trim()
    assert ctx.device_bytes() == 0
    w = nd_rows(ctx, lines)
    cols, vals = [((b"k",), S), ((b"j",), I)], [((b"v",), F)]
    parsed = ctx.device_bytes()
    got, _ = check(ctx, w, cols, vals, what="lifecycle")
    assert ctx.device_bytes() > parsed > 0  # the work arrays and the arena of the grouping are counted
    held = type(got)(got.rows, got.groups, got.key_bytes, got.key_kind, got.value_kind)
    ctx.select_records()
    ctx.extract_table([((b"k",), S), ((b"v",), F)])
    ctx.order_paths([((b"k",), S, False), ((b"v",), I, True)])
    ctx.marshal_rows()
    again = ctx.fetch_group_paths(held)  # materialised: it survives the selection, a table, an order and the marshaled rows
    assert np.array_equal(again.codes, got.codes) and again.keys[0] == got.keys[0] and np.array_equal(again.keys[1], got.keys[1])
    assert np.array_equal(bits(again.values[0][2]), bits(got.values[0][2]))
    ctx.trim()
    assert ctx.device_bytes() == 0  # the arena went with the others, and the grouping with it
    with pytest.raises(sjhip.ParseError) as e:
        ctx.fetch_group_paths(held)
    assert e.value.code == ERR_ARG and "no grouping" in str(e.value)
    nd_rows(ctx, lines)
    ctx.group_paths(cols, vals, fetch=False)
    nd_rows(ctx, lines)  # a parse drops it
    with pytest.raises(sjhip.ParseError) as e:
        ctx.fetch_group_paths(held)
    assert e.value.code == ERR_ARG and "no grouping" in str(e.value)
