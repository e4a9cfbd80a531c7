"""GPU: the row selection (sjhip_select_rows / sjhip_fetch_rows / sjhip_select_records) against the serial walk of
tests/rows_walk.py over the oracle's parse, and every call that runs on rows -- find_path, count_where_path, project_keys,
extract_path, extract_path_strings, the list columns, the tables -- against the walkers of the single products started from the
row's value: on the fixtures whose rows lie in an array, on every status, at the seams of the 2048-word tape tile and of the
record-count scans, on raw words that look like tags, at the limits of depth, on a sharded result, and through the lifecycle."""
import json

import numpy as np
import pytest

import column_walk as CW
import fixtures
import oracle_lib as O
import query_walk as Q
import rows_walk as RW
import table_walk as TW
from test_gpu_columns import RANDOM_PATHS, oracle_walk, random_nd
from test_gpu_parse import ctx  # noqa: F401
from test_gpu_tables import KINDS6, same_column
from test_rows_walk import STATUS_DOC, STATUS_PATH, STATUS_WANT

pytestmark = pytest.mark.gpu

F, I, U, B, S, SC = KINDS6
OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)
TILE = 2048  # TW_TILE of csrc/sj_tapewalk.h: 256 threads x 8 words


def check_selection(ctx, w, path):
    """select_rows + fetch_rows equal the serial walk; -> the RowWalk of the selection"""
    want_off, want_idx, want_st = RW.select_rows(w, path)
    nr, rows = ctx.select_rows(path)
    assert (nr, rows) == (len(want_st), len(want_idx)), (path, nr, rows)
    off, idx, st = ctx.fetch_rows(nr, rows)
    assert off.dtype == np.uint64 and idx.dtype == np.uint64 and st.dtype == np.uint8
    assert st.tolist() == want_st and off.tolist() == want_off, path
    assert np.array_equal(idx, np.array(want_idx, dtype=np.uint64)), path
    return RW.RowWalk(w, want_idx)


def check_queries(ctx, rw, paths, keys=None, eq=()):
    """every call that runs on rows, on the selection in force, against the walkers started from the rows' values"""
    n = len(rw.rows)
    for path in paths:
        got = ctx.find_path(*path)
        assert len(got) == n and got.tolist() == RW.find_path(rw, path), path
        assert ctx.count_where_path(path, ctx.OP_EXISTS) == RW.count_where_path(rw, path, Q.OP_EXISTS), path
        for kind in (F, I, U, B):
            same_column(kind, ctx.extract_path(path, kind), RW.column(rw, path, kind), ("extract_path", path, kind))
        for cvt in (False, True):
            same_column(S, ctx.extract_path_strings(path, cvt=cvt), RW.string_column(rw, path, cvt), ("strings", path, cvt))
        loff, vals, lst = ctx.extract_path_list(path, I)
        woff, wvals, wst = RW.list_column(rw, path, I)
        assert loff.tolist() == woff and lst.tolist() == wst and vals.view(np.uint64).tolist() == wvals, ("list", path)
        loff, soff, data, lst = ctx.extract_path_list_strings(path, cvt=True)
        assert (loff.tolist(), soff.tolist(), data, lst.tolist()) == RW.list_string_column(rw, path, True), ("list strings", path)
    for op, path, want in eq:
        assert ctx.count_where_path(path, op, want) == RW.count_where_path(rw, path, op, want), (op, path, want)
    if keys:
        got = ctx.project_keys(keys)
        assert got.shape == (n, len(keys))
        want = [[(j << 56) | v for j, v in row] + [2 ** 64 - 1] * (len(keys) - len(row)) for row in RW.project_keys(rw, keys)]
        assert got.tolist() == want
    columns = [(paths[j % len(paths)], KINDS6[j]) for j in range(6)]  # a six-kind table
    got = ctx.extract_table(columns)
    for c, (path, kind) in enumerate(columns):
        same_column(kind, got[c], TW.single(rw, path, kind), ("table", c, path, kind))
    return got


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_fixtures(ctx, copy):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy)
    rw = check_selection(ctx, w, (b"statuses",))
    want = json.loads(doc)["statuses"]
    assert len(rw.rows) == 100
    check_queries(ctx, rw, [(b"user", b"screen_name"), (b"id",), (b"retweeted",), (b"entities", b"hashtags"), (b"geo",)],
                  keys=[b"id", b"text", b"nope"], eq=[(ctx.OP_EQ_STRING, (b"lang",), b"ja"), (ctx.OP_EQ_INT, (b"retweet_count",), 0),
                                                       (ctx.OP_EQ_INT, (b"id",), want[3]["id"])])
    off, data, st = ctx.extract_path_strings((b"user", b"screen_name"))
    assert [data[off[k]:off[k + 1]].decode() for k in range(100)] == [s["user"]["screen_name"] for s in want]
    assert ctx.extract_path((b"id",), I)[0].tolist() == [s["id"] for s in want]
    assert ctx.count_where_path((b"lang",), ctx.OP_EQ_STRING, b"ja") == sum(s["lang"] == "ja" for s in want)

    doc = fixtures.load("github_events")  # the root array
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy)
    rw = check_selection(ctx, w, ())
    check_queries(ctx, rw, [(b"type",), (b"actor", b"login"), (b"payload", b"size"), (b"public",)], keys=[b"id", b"created_at"])
    off, data, st = ctx.extract_path_strings((b"actor", b"login"))
    assert [data[off[k]:off[k + 1]].decode() for k in range(len(st))] == [e["actor"]["login"] for e in json.loads(doc)]

    doc = fixtures.load("citm_catalog")
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy)
    rw = check_selection(ctx, w, (b"performances",))
    check_queries(ctx, rw, [(b"id",), (b"eventId",), (b"seatCategories",), (b"logo",)])
    assert ctx.extract_path((b"eventId",), U)[0].tolist() == [p["eventId"] for p in json.loads(doc)["performances"]]
    ctx.select_records()


def wrapped_random(seed, n):
    """random_nd's records as the items of NDJSON lines {"k":N,"items":[...]}, 0 to 7 of them per line"""
    recs = random_nd(seed, n).split(b"\n")
    lines, at, k = [], 0, 0
    while at < len(recs):
        take = (k * 5) % 8
        lines.append(b'{"k":%d,"items":[' % k + b",".join(recs[at:at + take]) + b"]}")
        at += take
        k += 1
    return b"\n".join(lines)


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_random_records_as_items(ctx, copy):
    doc = wrapped_random(11, 700)
    w = oracle_walk(doc, True, copy)
    ctx.parse(doc, ndjson=True, copy_strings=copy)
    rw = check_selection(ctx, w, (b"items",))
    assert len(rw.rows) == 700
    check_queries(ctx, rw, RANDOM_PATHS[:6], keys=[b"a", b"", b"c"], eq=[(ctx.OP_EQ_STRING, (b"a",), b"HOND"), (ctx.OP_EQ_INT, (b"b",), 1)])
    ctx.select_records()


# ---- statuses -------------------------------------------------------------------------------------------------------------------
def test_every_status(ctx):
    w = oracle_walk(STATUS_DOC, True, True)
    ctx.parse(STATUS_DOC, ndjson=True)
    rw = check_selection(ctx, w, STATUS_PATH)
    nr, rows = ctx.select_rows(STATUS_PATH)
    off, idx, st = ctx.fetch_rows(nr, rows)
    assert (off.tolist(), st.tolist()) == STATUS_WANT[:2] and "".join(chr(int(w.t[i]) >> 56) for i in idx) == STATUS_WANT[2]
    check_queries(ctx, rw, [(b"k",), (b"n",), (b"m",)], keys=[b"k"])
    assert ctx.extract_path((b"k",), I)[1].tolist() == [NOT_OBJECT] * 6 + \
        [TYPE, NOT_OBJECT, NOT_OBJECT, NOT_OBJECT, NOT_FOUND, NOT_OBJECT] + [NOT_OBJECT]
    check_selection(ctx, w, ())  # the root array of the third record
    check_selection(ctx, w, (b"a",))
    ctx.select_records()


def test_no_rows_at_all(ctx):
    doc = b'{"items":[]}\n{"items":null}\n{"x":[1,2]}\n[{"items":[1]}]'
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    want_table = ctx.extract_table([((b"x",), SC)])
    rw = check_selection(ctx, w, (b"items",))
    assert rw.rows == [] and ctx.select_rows((b"items",)) == (4, 0)
    assert len(ctx.find_path(b"x")) == 0 and ctx.count_where_path((b"x",), ctx.OP_EXISTS) == 0
    assert ctx.project_keys([b"x", b"y"]).shape == (0, 2)
    for kind in (F, I, U, B):
        vals, st = ctx.extract_path((b"x",), kind)
        assert len(vals) == 0 and len(st) == 0
    off, data, st = ctx.extract_path_strings((b"x",), cvt=True)
    assert off.tolist() == [0] and data == b"" and len(st) == 0
    loff, vals, lst = ctx.extract_path_list((b"x",), I)
    assert loff.tolist() == [0] and len(vals) == 0 and len(lst) == 0
    loff, soff, data, lst = ctx.extract_path_list_strings((b"x",))
    assert loff.tolist() == [0] and soff.tolist() == [0] and data == b"" and len(lst) == 0
    (vals, st), (off, data, st2) = ctx.extract_table([((b"x",), I), ((b"x",), S)])
    assert len(vals) == 0 and len(st) == 0 and off.tolist() == [0] and data == b"" and len(st2) == 0
    assert ctx.count_where(b"x", b"1") == 0  # (on records, whatever is selected)
    ctx.select_records()
    same_column(SC, ctx.extract_table([((b"x",), SC)])[0], want_table[0], "records again")


# ---- tile and wave seams ----------------------------------------------------------------------------------------------------------
RAW = {"[": 6557241057451442176, "{": 8863084066665136128, "]": 6701356245527298048, "}": 9007199254740992000,
       "l": 7782220156096217088, '"': 2449958197289549824}


def test_raw_values_look_like_tags():
    for tag, v in RAW.items():
        assert chr(v >> 56) == tag


def padded(first, items):
    """one document whose `items` array has its first element at tape word `first`: r { "p" [ pad ] "items" [ ..."""
    extra = first - 9
    assert extra >= 0
    pad = ["0"] * (extra // 2) + ["true"] * (extra % 2)
    return ('{"p":[%s],"items":[%s]}' % (",".join(pad), ",".join(items))).encode()


SEAM_ITEMS = ["true", "false", '{"a":1}', str(RAW["["]), '{"b":{"c":[1,{"d":2}]},"a":"s"}', '"str"', '[[1],[{"a":3}]]', "null",
              '{"a":%d}' % RAW["{"]]


@pytest.mark.parametrize("first", list(range(TILE - 14, TILE + 2)))
def test_rows_at_the_tile_boundary(ctx, first):
    """first = 2047: rows start at words 2047, 2048 and 2049 (true, false, an object); the other alignments put the object across
    the boundary (2043 .. 2047), the number's tag at the last word of the tile and its raw word -- which looks like '[' -- at the
    first of the next (2039), and every other word of the items there in turn"""
    doc = padded(first, SEAM_ITEMS)
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rw = check_selection(ctx, w, (b"items",))
    assert rw.rows[:4] == [first, first + 1, first + 2, first + 8] and len(rw.rows) == len(SEAM_ITEMS)
    if first in (TILE - 1, TILE - 9, TILE - 5):
        check_queries(ctx, rw, [(b"a",), (b"b", b"c")], keys=[b"a"])
    ctx.select_records()


SEAM_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)


@pytest.mark.parametrize("n", SEAM_COUNTS)
def test_row_counts_at_the_seams(ctx, n):
    items = ['{"a":{"b":%d},"s":"%s"}' % (r * 37 - 5, "t" * (r % 7) + str(r)) if r % 5 else '[%d,{"a":1}]' % r for r in range(n)]
    doc = ('{"n":%d,"items":[%s]}' % (n, ",".join(items))).encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rw = check_selection(ctx, w, (b"items",))
    assert len(rw.rows) == n
    got = ctx.extract_table([((b"a", b"b"), I), ((b"s",), S), ((b"a",), F)])
    for c, (path, kind) in enumerate([((b"a", b"b"), I), ((b"s",), S), ((b"a",), F)]):
        same_column(kind, got[c], TW.single(rw, path, kind), (n, c))
    assert len(ctx.find_path(b"a")) == n
    ctx.select_records()


# ---- raw words that look like tags ------------------------------------------------------------------------------------------------
def raw_doc():
    """Integers whose top byte is a tag, directly in the target array and inside element objects; the pad in front is a run of
    1100 integers whose tag AND raw word look like two-word tags (l): the tile that starts at word 2048 finds no anchor among the
    64 words in front of it and the global anchors decide; the 1300 direct elements at the end do the same to the tiles behind."""
    vals = list(RAW.values())
    items = []
    for k in range(300):
        v = vals[k % 6]
        items.append(str(v) if k % 3 == 0 else '{"a":%d,"b":[%d,{"a":%d}],"c":{"a":%d}}' % (v, vals[(k + 1) % 6], vals[(k + 2) % 6], v)
                     if k % 3 == 1 else "[%d,[%d]]" % (v, vals[(k + 4) % 6]))
    items += [str(RAW["l"])] * 1300
    return ('{"p":[%s],"items":[%s]}' % (",".join([str(RAW["l"])] * 1100), ",".join(items))).encode()


def check_raw_words(ctx):
    doc = raw_doc()
    w = oracle_walk(doc, False, True)
    run = [i for i in range(TILE - 70, TILE) if chr(w.t[i] >> 56) not in '"lud']
    assert run == [] and len(w.t) > 3 * TILE  # more than 64 words that look like two-word tags in front of a tile boundary
    ctx.parse(doc)
    rw = check_selection(ctx, w, (b"items",))
    assert len(rw.rows) == 1600
    check_queries(ctx, rw, [(b"a",), (b"c", b"a"), (b"b",)], eq=[(ctx.OP_EQ_INT, (b"a",), RAW["["]), (ctx.OP_EQ_INT, (b"c", b"a"), RAW["}"])])
    rw = check_selection(ctx, w, (b"p",))
    assert len(rw.rows) == 1100
    ctx.select_records()


def test_raw_words_that_look_like_tags(ctx):
    check_raw_words(ctx)


# ---- depth ------------------------------------------------------------------------------------------------------------------------
def test_depth(ctx):
    path = tuple(b"p%d" % j for j in range(16))
    deep = None
    for d in (1000, 500, 200, 100, 50):  # elements nested as deep as the parser allows (the oracle decides how deep that is)
        elem = b"[" * d + b'{"a":1}' + b"]" * d
        doc = b'{"a":7}'
        for key in reversed(path):
            doc = b'{"' + key + b'":' + doc + b'}'
        doc = doc.replace(b'{"a":7}', b'[{"a":1},' + elem + b',{"a":{"a":2}},' + b'{"a":' * d + b"3" + b"}" * d + b']')
        if O.parse(doc).rc == 0:
            deep = d
            break
    assert deep is not None
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rw = check_selection(ctx, w, path)
    assert len(rw.rows) == 4
    vals, st = ctx.extract_path((b"a",), I)
    assert vals.tolist() == [1, 0, 0, 0] and st.tolist() == [OK, NOT_OBJECT, TYPE, TYPE]
    check_queries(ctx, rw, [(b"a",), (b"a", b"a")])
    with pytest.raises(Exception):
        ctx.select_rows(path + (b"q",))  # 17 keys
    ctx.select_records()


# ---- a sharded result -----------------------------------------------------------------------------------------------------------------
def test_sharded_result_equals_whole():
    import sjhip
    recs = random_nd(13, 9000).split(b"\n")
    park = fixtures.load("parking-citations").split(b"\n")
    lines = []
    for k in range(0, 9000, 3):
        lines.append(b'{"order":%d,"items":[' % k + b",".join(recs[k:k + 3] + park[k % 900:k % 900 + 2]) + b"]}")
    doc = b"\n".join(lines)
    assert len(doc) > (2 << 20)
    columns = [((b"Make",), SC), ((b"a",), F), ((b"a", b"b"), S), ((b"Latitude",), I)]
    one = sjhip.Context(0)
    one.parse(doc, ndjson=True)
    nr, rows = one.select_rows((b"items",))
    want_rows = one.fetch_rows(nr, rows)
    want = one.extract_table(columns)
    with fixtures.nd_shard_limits(2 << 20, 1 << 20):
        many = sjhip.Context(0)
        many.parse(doc, ndjson=True)
    w = oracle_walk(doc, True, True)
    rw = check_selection(many, w, (b"items",))  # (row_index in merged tape indices: the oracle's are those of the whole tape)
    assert len(rw.rows) == 15000 == rows
    for a, b in zip(many.fetch_rows(nr, rows), want_rows):
        assert np.array_equal(a, b)
    got = many.extract_table(columns)
    for c, (path, kind) in enumerate(columns):
        same_column(kind, got[c], want[c], ("whole", c))
    assert many.count_where_path((b"Make",), many.OP_EQ_STRING, b"HOND") == one.count_where_path((b"Make",), one.OP_EQ_STRING, b"HOND") > 0
    many.select_records()
    assert len(many.find_path(b"order")) == 3000
    many.close()
    one.close()


# ---- lifecycle ----------------------------------------------------------------------------------------------------------------------
def test_lifecycle(ctx):
    import sjhip
    fresh = sjhip.Context(0)
    doc = b'{"o":1,"items":[{"s":"abc","n":1},{"s":"de","n":2.5}]}\n{"o":2,"items":[{"n":null}]}'
    columns = [((b"s",), S), ((b"n",), F)]
    fresh.parse(doc, ndjson=True)
    fresh.select_records()
    fresh.select_records()  # twice is fine, and so is nothing to give up
    with pytest.raises(sjhip.ParseError) as e:
        fresh.fetch_rows(2, 3)
    assert e.value.code == 5 and "no row selection" in str(e.value)
    before = fresh.extract_table([((b"o",), I), ((b"items",), SC)])
    base = fresh.device_bytes()
    assert fresh.select_rows((b"items",)) == (2, 3) and fresh.device_bytes() > base
    off, idx, st = fresh.fetch_rows(2, 3)
    assert off.tolist() == [0, 2, 3] and st.tolist() == [OK, OK]
    nr, nb = fresh.extract_table(columns, fetch=False)
    assert (nr, nb) == (3, [5, 0])
    fresh.select_records()  # the table built under the selection is materialised data
    with pytest.raises(sjhip.ParseError) as e:
        fresh.fetch_rows(2, 3)
    assert "no row selection" in str(e.value)
    off, data, st = fresh.fetch_table_column(0, nr, S, nb[0])
    assert off.tolist() == [0, 3, 5, 5] and data == b"abcde" and st.tolist() == [OK, OK, NOT_FOUND]
    vals, st = fresh.fetch_table_column(1, nr, F)
    assert vals.tolist() == [1.0, 2.5, 0.0] and st.tolist() == [OK, OK, NULL]
    after = fresh.extract_table([((b"o",), I), ((b"items",), SC)])  # without a selection: what it returned before
    same_column(I, after[0], before[0], "records again")
    same_column(SC, after[1], before[1], "records again")
    assert len(fresh.find_path(b"o")) == 2
    # a parse, a failed parse, trim: the selection is gone
    for drop in (lambda: fresh.parse(b'{"items":[1]}', ndjson=True), lambda: pytest.raises(sjhip.ParseError, fresh.parse, b'{"s":'),
                 fresh.trim):
        fresh.parse(doc, ndjson=True)
        fresh.select_rows((b"items",))
        drop()
        with pytest.raises(sjhip.ParseError) as e:
            fresh.fetch_rows(2, 3)
        assert "no row selection" in str(e.value)
    assert fresh.device_bytes() == 0  # (after trim)
    # a second selection replaces the first; a refused one (17 keys, a null count) leaves it
    fresh.parse(doc, ndjson=True)
    assert fresh.select_rows((b"items",)) == (2, 3)
    with pytest.raises(sjhip.ParseError):
        fresh.select_rows((b"k",) * 17)
    assert fresh.fetch_rows(2, 3)[0].tolist() == [0, 2, 3]
    assert fresh.select_rows((b"nope",)) == (2, 0)
    assert fresh.fetch_rows(2, 0)[2].tolist() == [NOT_FOUND, NOT_FOUND]
    L = sjhip.lib()  # any destination of the fetch may be null
    only = np.zeros(3, np.uint64)
    assert L.sjhip_fetch_rows(fresh._h, only.ctypes.data, None, None) == 0 and only.tolist() == [0, 0, 0]
    assert L.sjhip_fetch_rows(fresh._h, None, None, None) == 0
    fresh.close()
    # the selection survives the other products, the filter, the serializer and MarshalJSON, and they survive it
    doc = wrapped_random(5, 300)
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True, key_flags=True)
    rw = check_selection(ctx, w, (b"items",))
    nr, rows = ctx.select_rows((b"items",))
    text = ctx.marshal_json()
    filtered = ctx.filter_where(b"k", b"HOND")
    stream = ctx.serialize()
    assert ctx.count_where(b"k", b"x") == 0
    scol = ctx.extract_path_strings((b"a",), cvt=True)
    lcol = ctx.extract_path_list((b"b",), I)
    tnr, tnb = ctx.extract_table([((b"a",), SC), ((b"b",), I)], fetch=False)
    off, idx, st = ctx.fetch_rows(nr, rows)
    assert idx.tolist() == rw.rows
    same_column(S, scol, RW.string_column(rw, (b"a",), True), "column under the selection")
    assert lcol[0].tolist() == RW.list_column(rw, (b"b",), I)[0]
    snr, snb = ctx.extract_path_strings((b"a",), cvt=True, fetch=False)
    ctx.marshal_json(fetch=False)
    assert ctx.select_rows((b"items",)) == (nr, rows)  # a new selection: the materialised products stay
    same_column(S, ctx.fetch_path_strings(snr, snb), scol, "the string column after a selection")
    same_column(SC, ctx.fetch_table_column(0, tnr, SC, tnb[0]), TW.single(rw, (b"a",), SC), "the table after a selection")
    tl = np.empty(len(text), dtype=np.uint8)
    ctx._check(sjhip.lib().sjhip_fetch_marshaled(ctx._h, tl.ctypes.data))
    assert tl.tobytes() == text
    ctx.select_records()
    assert ctx.marshal_json() == text and np.array_equal(ctx.serialize(), stream)
