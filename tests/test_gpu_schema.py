"""GPU: the row schema (sjhip_row_schema / sjhip_fetch_row_schema) against the serial walk of tests/schema_walk.py over the oracle's
parse, exactly, in both copy modes unless noted: at the seams of the wave-level election of k_q_schema_insert (a wave's lanes all
one name, all distinct, alternating; as many distinct names as the election has rounds, and one and two more; a leader whose name
occurs once; a first occurrence in the last lane of one block whose repeats fill another), on names with one 64-bit hash, on
tables whose chains wrap, on names of every length around the hash word and the copy switch, on every type, on every parent
status, at a tile seam of the member walk, in composition with the selection -- which the call must leave exactly as it was,
with every product built before it --, through the lifecycle and the refusals, and on the fixtures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fixtures
import group_table as GT
import members_docs as D
import members_walk as MW
import rows_walk as RW
import schema_walk as SW
import unnest_walk as UW
import where_walk as WW
from test_gpu_columns import oracle_walk
from test_gpu_parse import ctx  # noqa: F401
from test_gpu_tables import KINDS6

pytestmark = pytest.mark.gpu

F, I, U, B, S, SC = KINDS6
OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the election's rounds, as the kernel has them
E = int(re.search(r"SCHEMA_ELECT_ROUNDS = (\d+);", open(os.path.join(ROOT, "simdjson-go_amd", "csrc", "query.hip")).read()).group(1))
VALUES = ("1", '"s"', "null", "true", "{}", "[1]", "2.5", "false", "18446744073709551615")  # a value of every type, by position


def check_schema(ctx, w, index, path):
    """row_schema on the selection in force (index: the walker's copy of its row index, None without one) equals the walker: the
    sizes, then the fetched dictionary, first rows and counts; -> the walker's result"""
    rw = UW.record_rows(w) if index is None else RW.RowWalk(w, index)
    want = SW.row_schema(rw, path)
    rows, status, members, names, first_row, counts = want
    s = ctx.row_schema(path, fetch=False)
    assert (s.rows, s.status.tolist(), s.members, s.n_names, s.name_bytes) == (rows, status, members, len(names), sum(map(len, names))), path
    assert s.status.dtype == np.uint64 and int(s.status.sum()) == rows
    ctx.fetch_row_schema(s)
    assert s.names == names, path
    assert s.name_offsets.tolist() == np.cumsum([0] + [len(n) for n in names]).tolist()
    assert s.first_row.dtype == np.uint64 and s.first_row.tolist() == first_row, path
    assert s.counts.dtype == np.uint64 and s.counts.shape == (len(names), 8) and s.counts.tolist() == counts, path
    assert int(s.counts.sum()) == members
    return want


def check_doc(ctx, doc, path, nd=False, select=None, copies=(True, False)):
    """the schema at `path` of the rows of select_rows(select) (None: of the records) in every copy mode -> the walker's result"""
    for copy in copies:
        w = oracle_walk(doc, nd, copy)
        ctx.parse(doc, ndjson=nd, copy_strings=copy)
        index = None
        if select is not None:
            sel = RW.select_rows(w, select)
            assert ctx.select_rows(select) == (len(sel[2]), len(sel[1]))
            index = sel[1]
        want = check_schema(ctx, w, index, path)
        ctx.select_records()
    return want


def one_object(names):
    return ('{"m":{%s}}' % ",".join('"%s":%s' % (n, VALUES[j % len(VALUES)]) for j, n in enumerate(names))).encode()


def one_member_rows(names):
    """row j is an object whose one member is names[j]: member numbers are row numbers"""
    return ('{"items":[%s]}' % ",".join('{"%s":%s}' % (n, VALUES[j % len(VALUES)]) for j, n in enumerate(names))).encode()


# ---- the election's seams ---------------------------------------------------------------------------------------------------------------
ELECTION_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)
PATTERNS = {"one name": lambda j: "same", "all distinct": lambda j: "n%d" % j, "two alternating": lambda j: ("even", "odd")[j & 1]}


def check_election_seam(ctx, n, pattern):
    names = [PATTERNS[pattern](j) for j in range(n)]
    want = check_doc(ctx, one_object(names), (b"m",))
    assert want[2] == n and want[3] == [x.encode() for x in dict.fromkeys(names)]


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("n", ELECTION_COUNTS)
def test_election_seams(ctx, n, pattern):
    check_election_seam(ctx, n, pattern)


def check_election_rounds(ctx):
    """E, E + 1 and E + 2 distinct names cycling inside every wave: with more names than rounds the last ones probe for themselves"""
    for k in (max(E, 1), E + 1, E + 2):
        names = ["c%d" % (j % k) for j in range(200)]
        want = check_doc(ctx, one_object(names), (b"m",))
        assert len(want[3]) == k and [sum(c) for c in want[5]] == [names.count("c%d" % i) for i in range(k)]
    # blocks of equal names, so that late rounds meet lanes that are still pending from the first
    names = ["b%d" % (j // 9) for j in range(300)]
    assert len(check_doc(ctx, one_object(names), (b"m",))[3]) == 34


def check_leaders(ctx):
    # a wave whose leader's name occurs only once, in every wave of three blocks; then once in the whole input
    names = ["solo%d" % (j // 64) if j % 64 == 0 else "x" for j in range(768)]
    want = check_doc(ctx, one_member_rows(names), (), select=(b"items",))
    assert want[3][:2] == [b"solo0", b"x"] and want[4][:3] == [0, 1, 64] and sum(want[5][1]) == 768 - 12
    names = ["only"] + ["x"] * 63
    assert check_doc(ctx, one_member_rows(names), (), select=(b"items",))[4] == [0, 1]
    # a name whose first occurrence is the last lane of block 0 and whose next occurrences fill block 2
    names = ["a%d" % j for j in range(255)] + ["late"] + ["b%d" % (j % 7) for j in range(256)] + ["late"] * 256 + ["tail"]
    want = check_doc(ctx, one_member_rows(names), (), select=(b"items",))
    k = want[3].index(b"late")
    assert k == 255 and want[4][k] == 255 and sum(want[5][k]) == 257 and want[4][want[3].index(b"tail")] == 768


def test_election_rounds(ctx):
    check_election_rounds(ctx)


def test_leaders_and_first_occurrences(ctx):
    check_leaders(ctx)


# ---- equal hashes -------------------------------------------------------------------------------------------------------------------------
COLLIDING = {"16 bytes": (16, False), "a shared tail": (21, False), "behind an equal first word": (24, True)}


def check_equal_hashes(ctx, variant):
    length, same_first = COLLIDING[variant]
    keys = [k.decode() for k in GT.colliding_strings(4, length, same_first)]
    assert len({GT.hash_bytes(k.encode()) for k in keys}) == 1
    interleaved = [keys[p] if p is not None else "other%d" % j for j, p in enumerate(GT.COLLIDE_PATTERN * 8)]  # inside one wave
    spread = [keys[(j // 70) % 4] for j in range(70 * 8)]                                                       # ... and wave after wave
    for names in (interleaved, spread, interleaved + spread):
        want = check_doc(ctx, one_member_rows(names), (), select=(b"items",))
        for k in keys:  # four names with their own counts and first rows
            at = want[3].index(k.encode())
            assert sum(want[5][at]) == names.count(k) and want[4][at] == names.index(k)


@pytest.mark.parametrize("variant", list(COLLIDING))
def test_equal_hashes_stay_apart(ctx, variant):
    check_equal_hashes(ctx, variant)


# ---- table seams ---------------------------------------------------------------------------------------------------------------------------
def check_table_wrap(ctx, cap, members):
    """names homed at the last slot of a table of `cap` slots: the chain wraps mask -> 0, and every repeat finds its slot by probing"""
    assert GT.capacity(members) == cap
    homed = [k.decode() for k in GT.string_keys_at(cap - 1, cap - 1, 5, 12)]
    names = [homed[GT.REPEAT_PATTERN[j % 32] % 5] if j % 3 else "f%d" % (j % 11) for j in range(members)]
    want = check_doc(ctx, one_object(names), (b"m",))
    assert [sum(want[5][want[3].index(k.encode())]) for k in homed] == [names.count(k) for k in homed]
    keys = [n.encode() for n in names]  # (in the reverse order the larger member of every name claims first: slots reached by probing are lowered)
    assert GT.model(keys, cap - 1).wrapped and GT.model(keys, cap - 1, order=range(members - 1, -1, -1)).lowered_probed


@pytest.mark.parametrize("cap,members", [(64, 32), (128, 64), (2048, 1000)])
def test_chains_wrap(ctx, cap, members):
    check_table_wrap(ctx, cap, members)


def test_capacity_step(ctx):
    for n in (32, 33):
        assert GT.capacity(n) == (64 if n == 32 else 128)
        assert len(check_doc(ctx, one_object(["d%d" % j for j in range(n)]), (b"m",))[3]) == n


# ---- names -----------------------------------------------------------------------------------------------------------------------------------
def check_names(ctx):
    names = [""]
    for ln in list(range(1, 130)) + [512, 5000]:  # each with a twin that differs in its last byte
        names += ["n" * (ln - 1) + "a", "n" * (ln - 1) + "b", "n" * (ln - 1) + "a"]
    want = check_doc(ctx, one_object(names), (b"m",))
    assert len(want[3]) == 1 + 2 * 131 and [sum(c) for c in want[5]][1:] == [2, 1] * 131
    # escaped spellings of one name, names that need unescaping, duplicates inside one object
    doc = b'{"m":{"ab":1,"\\u0061b":"s","a\\u0062":null,"AB":1,"a\\"b":1,"a\\\\b":2,"\\u00e9\\n":3,"dup":1,"dup":[],"dup":{},"":0,"":1.5}}'
    want = check_doc(ctx, doc, (b"m",))
    assert want[3] == [b"ab", b"AB", b'a"b', b"a\\b", "é\n".encode(), b"dup", b""] and [sum(c) for c in want[5]] == [3, 1, 1, 1, 1, 3, 2]
    check_doc(ctx, D.names_doc(), (b"m",))


def test_names(ctx):
    check_names(ctx)


# ---- types -----------------------------------------------------------------------------------------------------------------------------------
def check_types(ctx):
    doc = b'{"k":null,"k":"s","k":-1,"k":9223372036854775807,"k":9223372036854775808,"k":1e0,"k":true,"k":false,"k":{"k":1},"k":[{"k":2}]}'
    assert check_doc(ctx, doc, ())[5] == [[1, 1, 2, 1, 1, 2, 1, 1]]
    doc = b'[{"b":true},{"b":false},{"n":9223372036854775807},{"n":9223372036854775808},{"n":1e0}]'
    want = check_doc(ctx, doc, (), select=())
    assert want[3] == [b"b", b"n"] and want[5] == [[0, 0, 0, 0, 0, 2, 0, 0], [0, 0, 1, 1, 1, 0, 0, 0]] and want[4] == [0, 2]
    for n in (31, 32, 33, 300):  # name * 8 + type crosses a sort digit
        names = ["t%d" % (j % n) for j in range(3 * n + 5)]
        want = check_doc(ctx, one_object(names), (b"m",), copies=(True,))
        assert len(want[3]) == n and sum(1 for c in want[5] for x in c if x) > n


def test_types(ctx):
    check_types(ctx)


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------
def check_rows(ctx):
    want = check_doc(ctx, D.STATUS_DOC, (b"a",), nd=True, select=(b"o",))
    assert want[1] == [4, 1, 2, 3, 1, 0] and want[3] == [b"x", b"y", b"", b'a"b', "é\n".encode(), b"d"]
    assert check_doc(ctx, D.STATUS_DOC, (b"o",), nd=True)[:3] == (4, [0, 0, 0, 3, 1, 0], 0)
    assert check_doc(ctx, D.KINDS_DOC, (), select=())[1] == [4, 0, 0, 4, 1, 0]  # rows that are scalars and arrays
    check_doc(ctx, D.KINDS_DOC, (b"k",), select=())
    assert check_doc(ctx, b'[{},{},{"a":{}},{}]', (), select=())[2:4] == (1, [b"a"])  # empty objects
    assert check_doc(ctx, b'[{},{},{}]', (), select=())[:3] == (3, [3, 0, 0, 0, 0, 0], 0)  # no members
    assert check_doc(ctx, b'{"items":[],"x":{"a":1}}', (), select=(b"items",))[:3] == (0, [0] * 6, 0)  # no rows
    assert check_doc(ctx, b'{"m":{}}\n{"m":null}\n{"x":{"a":1}}\n[{"m":{"a":1}}]', (b"m",), nd=True)[:3] == (4, [1, 1, 1, 0, 1, 0], 0)


def check_0_to_7(ctx):
    want = check_doc(ctx, D.nested_lines(300), (b"o",), nd=True, select=(b"items",))
    assert want[:3] == (1050, [840, 30, 0, 107, 73, 0], 2886) and len(want[3]) == 1675


def check_tile_seam(ctx, key_at):
    doc = D.seam_doc(key_at)
    w = oracle_walk(doc, False, True)
    m = MW.unnest_members(UW.record_rows(w), (b"m",))[1]
    assert m[0] - 2 == key_at
    assert check_doc(ctx, doc, (b"m",), copies=(True,))[2] == len(m) == 3060


def test_rows(ctx):
    check_rows(ctx)


def test_0_to_7_parents_of_0_to_7_members(ctx):
    check_0_to_7(ctx)


@pytest.mark.parametrize("key_at", [D.TILE - 1, D.TILE, D.TILE + 1])
def test_member_walk_tile_seam(ctx, key_at):
    check_tile_seam(ctx, key_at)


# ---- composition: the call reads the selection and leaves it, and every product, as they were ---------------------------------------------
def snapshot(ctx, sel, parents=None):
    """what the selection of `sel` = (records, rows) and the parents product of (parents, its rows) read back as"""
    out = list(ctx.fetch_rows(*sel))
    if parents is not None:
        out += list(ctx.fetch_row_parents(*parents))
    return out


def same(a, b):
    assert len(a) == len(b) and all(x == y if isinstance(x, (bytes, list)) else np.array_equal(x, y) for x, y in zip(a, b))


def built_before(ctx, sel, parents, columns, group):
    """a table and a grouping built on the selection in force -> a reader of everything a schema call must leave alone: the
    selection, the parents product, the table's columns and the grouping, as flat lists of arrays"""
    n_table, text = ctx.extract_table(columns, fetch=False)
    g = ctx.group_path(group, S, fetch=False)

    def read():
        out = snapshot(ctx, sel, parents)
        for c, (_, kind) in enumerate(columns):
            out += list(ctx.fetch_table_column(c, n_table, kind, text[c]))
        k = ctx.fetch_groups(type(g)(g.rows, g.groups, g.key_bytes, g.key_kind, None))
        return out + [k.keys, k.codes, k.group_rows, k.first_row, k.status]
    return read


def check_composition(ctx, copy):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy)
    rows = RW.select_rows(w, (b"statuses",))
    n = len(rows[1])
    assert ctx.unnest_rows((b"statuses",)) == (1, 1, n)  # the statuses as the rows, with a parents product to leave alone
    assert ctx.fetch_rows(1, n)[1].tolist() == rows[1]
    columns, group, parents = [((b"id",), I), ((b"user", b"screen_name"), S)], (b"user", b"lang"), (1, n)
    read = built_before(ctx, (1, n), parents, columns, group)
    before = read()
    assert len(before) == 3 + 3 + 2 + 3 + 5 and len(before[-5]) > 3
    for path in ((), (b"user",)):
        want = check_schema(ctx, w, rows[1], path)
        assert want[1][OK] == n and len(want[3]) > 20
        same(read(), before)
    # after a narrowing: the schema of what is left; the selection, the parents, a table and a grouping built on the kept rows stay
    kept = ctx.where_path((b"retweet_count",), WW.OP_GE_INT, 1)
    assert kept[0] == 1 and 0 < kept[1] < n
    read = built_before(ctx, kept, parents, columns, group)
    before = read()
    assert set(before[1].tolist()) < set(rows[1]) and len(before[6]) == kept[1]
    check_schema(ctx, w, before[1].tolist(), (b"user",))
    same(read(), before)
    # ... and after an order with a limit, with the order itself
    o = ctx.order_path((b"id",), I, limit=7)
    read = built_before(ctx, (1, 7), parents, columns, group)
    before = read()
    check_schema(ctx, w, before[1].tolist(), (b"entities",))
    same(read(), before)
    again = ctx.fetch_order(type(o)(o.records, o.rows, o.kind))
    assert np.array_equal(again.order, o.order) and np.array_equal(again.values, o.values)
    ctx.select_records()
    # under unnest_members (a map of maps, an empty path): the member selection keeps its names, the parents stay
    w = oracle_walk(D.MAP_OF_MAPS, False, copy)
    ctx.parse(D.MAP_OF_MAPS, copy_strings=copy)
    m = MW.unnest_members(UW.record_rows(w), (b"m",))
    assert ctx.unnest_members((b"m",)) == (1, 1, 6)
    read = built_before(ctx, (1, 6), (1, 6), [((b"x",), I), ((b"y",), SC)], (b"z", b"w"))
    before, names = read(), ctx.extract_row_names()
    want = check_schema(ctx, w, m[1], ())
    assert want[1] == [4, 0, 0, 2, 0, 0] and want[3] == [b"x", b"y", b"z"] and want[4] == [0, 0, 2] and want[5][1][2] == 2
    same(read(), before)
    assert ctx.extract_row_names()[1] == names[1] == b"abcdea"  # (still a selection of members)
    ctx.select_records()


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_composition_leaves_everything_alone(ctx, copy):
    check_composition(ctx, copy)


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------------------
def check_fixtures(ctx, copy):
    doc = fixtures.load("citm_catalog")
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy)
    m = MW.unnest_members(UW.record_rows(w), (b"events",))
    assert ctx.unnest_members((b"events",)) == (1, 1, 184)
    assert check_schema(ctx, w, m[1], ())[2] == 184 * 8
    ctx.select_records()
    assert check_schema(ctx, w, None, (b"areaNames",))[2] > 10
    doc = fixtures.load("update-center")
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy)
    m = MW.unnest_members(UW.record_rows(w), (b"plugins",))
    ctx.unnest_members((b"plugins",))
    assert check_schema(ctx, w, m[1], ())[2] > 5000
    ctx.select_records()
    doc = D.parking_lines()
    w = oracle_walk(doc, True, copy)
    ctx.parse(doc, ndjson=True, copy_strings=copy)
    want = check_schema(ctx, w, None, ())
    assert want[0] == 400 and 15 < len(want[3]) < 30 and want[4] == [0] * 19 + want[4][19:]
    doc = fixtures.load("github_events")
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy)
    rows = RW.select_rows(w, ())
    ctx.select_rows(())
    for path in ((), (b"payload",), (b"actor",)):
        check_schema(ctx, w, rows[1], path)
    ctx.select_records()


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_fixtures(ctx, copy):
    check_fixtures(ctx, copy)


# ---- the lifecycle and the refusals ------------------------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals():
    import sjhip
    fresh = sjhip.Context(0)
    with pytest.raises(sjhip.ParseError) as e:  # no result on the device
        fresh.row_schema(())
    assert e.value.code == 5
    doc = b'{"o":1,"m":{"a":1,"b":[2],"a":{"c":3}}}\n{"o":2,"m":null}'
    fresh.parse(doc, ndjson=True)
    with pytest.raises(sjhip.ParseError) as e:
        fresh.fetch_row_schema(sjhip.Schema(2, None, 3, 2, 2))
    assert "no row schema on the device" in str(e.value) and e.value.code == 5
    base = fresh.device_bytes()
    s = fresh.row_schema((b"m",))
    assert (s.rows, s.status.tolist(), s.members, s.names) == (2, [1, 0, 0, 0, 1, 0], 3, [b"a", b"b"]) and fresh.device_bytes() > base
    assert s.first_row.tolist() == [0, 0] and s.counts.tolist() == [[0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0, 0, 1]]
    # SJHIP_ERR_ARG touches nothing, the previous schema included: a bad path, a null size pointer
    L, h = sjhip.lib(), fresh._h
    with pytest.raises(sjhip.ParseError):
        fresh.row_schema((b"k",) * 17)
    lens, st = (C.c_uint32 * 1)(1), (C.c_uint64 * 6)()
    a, b, c, d = C.c_size_t(7), C.c_uint64(7), C.c_size_t(7), C.c_size_t(7)
    assert L.sjhip_row_schema(h, b"m", lens, 1, None, st, C.byref(b), C.byref(c), C.byref(d)) == 5
    assert b"sjhip_row_schema: a null size pointer" in L.sjhip_last_error(h)
    assert L.sjhip_row_schema(h, b"m", lens, 1, C.byref(a), None, C.byref(b), C.byref(c), C.byref(d)) == 5
    assert L.sjhip_row_schema(h, None, None, 1, C.byref(a), st, C.byref(b), C.byref(c), C.byref(d)) == 5
    kept = fresh.fetch_row_schema(sjhip.Schema(2, s.status, 3, 2, 2))
    assert kept.names == s.names and np.array_equal(kept.counts, s.counts)
    # any destination of the fetch may be null
    counts = np.zeros(16, dtype=np.uint64)
    assert L.sjhip_fetch_row_schema(h, None, None, None, counts.ctypes.data) == 0 and counts.reshape(2, 8).tolist() == s.counts.tolist()
    assert L.sjhip_fetch_row_schema(h, None, None, None, None) == 0
    # it survives the selection and the other products, and they survive it; the next call replaces it, an empty one included
    fresh.select_rows((b"m", b"b"))
    fresh.extract_path_strings((b"x",), cvt=True)
    fresh.marshal_json()
    assert fresh.fetch_row_schema(sjhip.Schema(2, s.status, 3, 2, 2)).names == s.names
    empty = fresh.row_schema(())  # the rows are numbers now
    assert (empty.rows, empty.status.tolist(), empty.members, empty.names) == (1, [0, 0, 0, 1, 0, 0], 0, []) and empty.counts.shape == (0, 8)
    assert empty.name_offsets.tolist() == [0] and fresh.fetch_rows(2, 1)[1].tolist()
    fresh.select_records()
    # a parse and trim drop it
    for drop in (lambda: fresh.parse(b'{"m":{"a":1}}', ndjson=True), fresh.trim):
        fresh.parse(doc, ndjson=True)
        assert fresh.row_schema(()).names == [b"o", b"m"]
        drop()
        with pytest.raises(sjhip.ParseError) as e:
            fresh.fetch_row_schema(sjhip.Schema(2, None, 4, 2, 2))
        assert "no row schema on the device" in str(e.value)
    assert fresh.device_bytes() == 0
    fresh.close()


def test_a_sharded_result_is_refused():
    import sjhip
    doc = D.sharded_lines()
    with fixtures.nd_shard_limits(2 << 20, 1 << 20):
        many = sjhip.Context(0)
        many.parse(doc, ndjson=True)
    with pytest.raises(sjhip.ParseError) as e:
        many.row_schema((b"m",))
    assert e.value.code == 5 and "is sharded" in str(e.value) and "sjhip_row_schema" in str(e.value)
    assert many.unnest_members((b"m",))[0] == 9000  # (the result itself is whole and well)
    many.select_records()
    many.close()
    one = sjhip.Context(0)
    one.parse(doc, ndjson=True)
    s = one.row_schema((b"m",), fetch=False)
    assert s.rows == 9000 and s.members > 30000 and s.n_names > 7000
    one.close()
