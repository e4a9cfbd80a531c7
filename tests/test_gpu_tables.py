"""GPU: tables (sjhip_extract_table + sjhip_fetch_table_column) -- columns at several paths from one walk of every record --
against the single-column calls on the same context (sjhip_extract_path / sjhip_extract_path_strings, kernels the tables leave
untouched) and against the restated conversions of tests/column_walk.py over the oracle's parse: values as bits, statuses,
offsets and bytes; at the wave, block and scan-tile seams; at the limits of depth and width; on a sharded result; and the
lifecycle of the table among the other products of a context."""
import ctypes as C

import numpy as np
import pytest

import column_walk as CW
import fixtures
import table_walk as TW
from test_gpu_columns import RANDOM_PATHS, oracle_walk, random_nd
from test_gpu_parse import ctx  # noqa: F401
from test_query_walk import FINDPATH_INPUT
from test_table_walk import DEEP_COLUMNS, DEEP_DOC, DEEP_PATH, EDGE_COLUMNS, EDGE_DOC, PREFIX_COLUMNS, WIDE_COLUMNS, WIDE_DOC

pytestmark = pytest.mark.gpu

F, I, U, B, S, SC = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT, CW.COL_BOOL, TW.COL_STRING, TW.COL_STRING_CVT
KINDS6 = (F, I, U, B, S, SC)


def is_string(kind):
    return kind in (S, SC)


def same_column(kind, got, want, what):
    """got: what the device returned; want: column_walk's lists, or another device column"""
    if is_string(kind):
        (off, data, st), (woff, wdata, wst) = got, want
        assert off.dtype == np.uint64 and np.array_equal(off, np.asarray(woff, dtype=np.uint64)), what
        assert data == wdata, what
    else:
        (vals, st), (wvals, wst) = got, want
        assert vals.dtype == (np.uint8 if kind == B else {F: np.float64, I: np.int64, U: np.uint64}[kind]), what
        bits = np.uint8 if kind == B else np.uint64
        wv = wvals.view(bits) if isinstance(wvals, np.ndarray) else np.asarray(wvals, dtype=bits)
        assert np.array_equal(vals.view(bits), wv), what
    assert st.dtype == np.uint8 and np.array_equal(st, np.asarray(wst, dtype=np.uint8)), what


def single_call(ctx, path, kind):
    if is_string(kind):
        return ctx.extract_path_strings(path, cvt=kind == SC)
    return ctx.extract_path(path, kind)


def check_table(ctx, w, columns, singles=True):
    got = ctx.extract_table(columns)
    assert len(got) == len(columns)
    for c, (path, kind) in enumerate(columns):
        same_column(kind, got[c], TW.single(w, path, kind), ("column_walk", c, path, kind))
        if singles:
            same_column(kind, got[c], single_call(ctx, path, kind), ("single call", c, path, kind))
    return got


# ---- random records ---------------------------------------------------------------------------------------------------------------
_walks = {}


def random_walk(copy):
    if copy not in _walks:
        _walks[copy] = (random_nd(11, 3000), oracle_walk(random_nd(11, 3000), True, copy))
    return _walks[copy]


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_random_records(ctx, copy):
    doc, w = random_walk(copy)
    ctx.parse(doc, ndjson=True, copy_strings=copy)
    # the paths split into tables that cycle through all six kinds
    for first in range(6):
        for lo in range(0, len(RANDOM_PATHS), 3):
            columns = [(p, KINDS6[(first + j) % 6]) for j, p in enumerate(RANDOM_PATHS[lo:lo + 3])]
            check_table(ctx, w, columns, singles=first < 2)
    check_table(ctx, w, [(p, KINDS6[j % 6]) for j, p in enumerate(RANDOM_PATHS)])           # all nine paths
    check_table(ctx, w, [((b"a", b"b"), I), ((b"a", b"b"), SC)])                            # one path twice
    check_table(ctx, w, [((b"a",), SC), ((b"a", b"b"), SC), ((b"a", b"b", b"c"), SC), ((b"a", b""), F)])  # prefixes


def test_hand_written_edges(ctx):
    for copy in (True, False):
        for doc, columns in ((EDGE_DOC, EDGE_COLUMNS), (WIDE_DOC, WIDE_COLUMNS)):
            ctx.parse(doc, ndjson=True, copy_strings=copy)
            check_table(ctx, oracle_walk(doc, True, copy), columns)


# ---- seams: the wave (64), the block (256) and the scan tile (QTILE = 1024 over n + 1 entries) -------------------------------------
SEAM_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
SEAM_COLUMNS = [((b"a", b"b"), I), ((b"s",), S), ((b"a",), F)]


def seam_doc(n, variant):
    lines = []
    long_at = min(n, 64) - 1  # the last record of the first wave (of the only one, when it is not full)
    for r in range(n):
        text = "" if variant == "empty" else "t" * (r % 7) + str(r)
        if variant == "long" and r == long_at:
            text = "L" * 3000
        if variant == "none ok":
            lines.append('{"a":{"b":"x"},"s":%d,"a":1}' % r)
        else:
            lines.append('{"a":{"b":%d},"s":"%s","a":1}' % (r * 37 - 5, text))
    return "\n".join(lines).encode()


@pytest.mark.parametrize("variant", ["plain", "empty", "long", "none ok"])
def test_seams(ctx, variant):
    for n in SEAM_COUNTS:
        doc = seam_doc(n, variant)
        ctx.parse(doc, ndjson=True)
        (vals, st_i), (off, data, st_s), (fl, st_f) = check_table(ctx, oracle_walk(doc, True, True), SEAM_COLUMNS, singles=n in (65, 1025))
        assert len(vals) == n and len(off) == n + 1 and np.all(st_f == CW.COL_TYPE) and not fl.any()
        if variant == "none ok":
            assert np.all(st_i == CW.COL_TYPE) and np.all(st_s == CW.COL_TYPE) and not off.any() and data == b""
        else:
            assert np.all(st_i == CW.COL_OK) and np.all(st_s == CW.COL_OK) and vals[-1] == (n - 1) * 37 - 5
        if variant == "empty":
            assert not off.any() and data == b""
        if variant == "long":
            assert b"L" * 3000 in data


# ---- depth and width ----------------------------------------------------------------------------------------------------------------
def test_depth_and_width(ctx):
    assert len(DEEP_COLUMNS) == 16 and sum(len(p) for p, _ in DEEP_COLUMNS) == 32 and len(DEEP_PATH) == 16
    for copy in (True, False):
        ctx.parse(DEEP_DOC, ndjson=True, copy_strings=copy)
        w = oracle_walk(DEEP_DOC, True, copy)
        got = check_table(ctx, w, DEEP_COLUMNS)
        assert got[0][0].tolist()[:1] == [42] and got[0][1].tolist() == [CW.COL_OK, CW.COL_NOT_OBJECT, CW.COL_TYPE, CW.COL_NOT_FOUND]
        got = check_table(ctx, w, PREFIX_COLUMNS)  # the paths of 10, 1, 9, 4 and 8 keys
        # the second record has level 9 as a string: everything below it is NOT_OBJECT, everything above is what it is in the first
        st = [[int(col[-1][r]) for col in got] for r in (0, 1)]
        assert st[0] == [CW.COL_TYPE] * 5
        assert st[1] == [CW.COL_NOT_OBJECT, CW.COL_TYPE, CW.COL_OK, CW.COL_TYPE, CW.COL_TYPE]
        assert got[2][1] == b"level 9 is a string"


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def test_fixtures(ctx):
    park = fixtures.load("parking-citations") * 7
    columns = [((b"Make",), S), ((b"Color",), S), ((b"Latitude",), S), ((b"Make",), SC), ((b"Color",), SC), ((b"Latitude",), SC),
               ((b"Make",), F)]
    for copy in (True, False):
        ctx.parse(park, ndjson=True, copy_strings=copy)
        got = check_table(ctx, oracle_walk(park, True, copy), columns)
        assert np.all(got[6][1] == CW.COL_TYPE)  # every value of the parking records is a string
    tw = fixtures.load("twitter")
    ctx.parse(tw)
    got = check_table(ctx, oracle_walk(tw, False, True), [((b"search_metadata", b"count"), I), ((b"search_metadata", b"max_id_str"), S),
                                                           ((b"search_metadata",), I)])
    assert got[0][0].tolist() == [100] and got[2][1].tolist() == [CW.COL_TYPE]
    image = [(b"Image", b"Thumbnail", b"Width"), (b"Image", b"Thumbnail", b"Url"), (b"Image", b"IDs"), (b"Alt",), (b"Image", b"Animated"),
             (b"Image", b"IDs", b"0")]
    for copy in (True, False):
        ctx.parse(FINDPATH_INPUT, copy_strings=copy)
        w = oracle_walk(FINDPATH_INPUT, False, copy)
        got = check_table(ctx, w, [(p, SC) for p in image] + [(p, I) for p in image] + [(image[4], B)])
        assert got[0][1] == b"100" and got[6][0].tolist() == [100]  # ExampleIter_FindElement


# ---- a sharded result -----------------------------------------------------------------------------------------------------------------
def test_sharded_result_equals_whole():
    import sjhip
    park = fixtures.load("parking-citations")
    doc = park * 4 + random_nd(13, 9000) + b"\n" + park * 3
    assert len(doc) > (2 << 20)
    columns = [((b"Make",), SC), ((b"a",), F), ((b"a", b"b"), S), ((b"Latitude",), I)]
    one = sjhip.Context(0)
    for copy in (True, False):
        one.parse(doc, ndjson=True, copy_strings=copy)
        want = one.extract_table(columns)
        with fixtures.nd_shard_limits(2 << 20, 1 << 20):
            many = sjhip.Context(0)
            many.parse(doc, ndjson=True, copy_strings=copy)
        got = check_table(many, oracle_walk(doc, True, copy), columns, singles=False)
        for c, (path, kind) in enumerate(columns):
            same_column(kind, got[c], want[c], ("whole", c, copy))
        many.close()
    one.close()


# ---- lifecycle ----------------------------------------------------------------------------------------------------------------------
def test_lifecycle(ctx):
    import sjhip
    fresh = sjhip.Context(0)
    doc = b'{"s":"abc","n":1}\n{"s":"de","n":2.5}\n{"n":null}'
    columns = [((b"s",), S), ((b"n",), F)]
    fresh.parse(doc, ndjson=True)
    with pytest.raises(sjhip.ParseError) as e:  # no table yet
        fresh.fetch_table_column(0, 3, S, 5)
    assert e.value.code == 5 and "no table" in str(e.value)
    base = fresh.device_bytes()
    nr, nb = fresh.extract_table(columns, fetch=False)
    assert (nr, nb) == (3, [5, 0]) and fresh.device_bytes() > base
    with pytest.raises(sjhip.ParseError) as e:  # a column the table does not have
        fresh.fetch_table_column(2, 3, F)
    assert e.value.code == 5 and "column 2" in str(e.value)
    off, data, st = fresh.fetch_table_column(0, nr, S, nb[0])
    assert off.tolist() == [0, 3, 5, 5] and data == b"abcde" and st.tolist() == [0, 0, CW.COL_NOT_FOUND]
    vals, st = fresh.fetch_table_column(1, nr, F)
    assert vals.tolist() == [1.0, 2.5, 0.0] and st.tolist() == [0, 0, CW.COL_NULL]
    # a parse, a failed parse, trim: the table is gone
    for drop in (lambda: fresh.parse(b'{"s":"z"}', ndjson=True), lambda: pytest.raises(sjhip.ParseError, fresh.parse, b'{"s":'),
                 fresh.trim):
        fresh.parse(doc, ndjson=True)
        fresh.extract_table(columns, fetch=False)
        drop()
        with pytest.raises(sjhip.ParseError) as e:
            fresh.fetch_table_column(0, 3, S, 5)
        assert "no table" in str(e.value)
    assert fresh.device_bytes() == 0  # (after trim)
    # the limits and the kinds, through the C ABI
    fresh.parse(doc, ndjson=True)
    for bad, word in (([], "1 to 16 columns"), ([((b"s",), S)] * 17, "1 to 16 columns"), ([((b"s",), 6)], "kind"), ([((), S)], "no key"),
                      ([((b"k",) * 17, S)], "more than 16 keys"), ([((b"k",) * 11, S)] * 3, "more than 32 keys"),
                      ([((b"x" * 1025,), S)], "1024 bytes")):
        with pytest.raises(sjhip.ParseError) as e:
            fresh.extract_table(bad)
        assert e.value.code == 5 and word in str(e.value), (word, str(e.value))
    L = sjhip.lib()
    blob, lens, n = fresh._keys([b"s"])
    cnt, ne = C.c_size_t(0), C.c_size_t(0)
    vals, st = np.zeros(4, np.float64), np.zeros(4, np.uint8)
    for kind in (S, SC):  # kinds of table columns only
        assert L.sjhip_extract_path(fresh._h, blob, lens, n, kind, vals.ctypes.data, st.ctypes.data, 4, C.byref(cnt)) == 5
        assert L.sjhip_extract_path_list(fresh._h, blob, lens, n, kind, C.byref(cnt), C.byref(ne)) == 5
    fresh.close()
    # the other products between extract and fetch leave the table alone, and it leaves them alone
    big = fixtures.load("parking-citations")
    ctx.parse(big, ndjson=True, key_flags=True)
    w = oracle_walk(big, True, True)
    columns = [((b"Make",), SC), ((b"Fine",), I), ((b"Color",), S)]
    want = [TW.single(w, p, k) for p, k in columns]
    nr, nb = ctx.extract_table(columns, fetch=False)
    text = ctx.marshal_json()
    ctx.filter_where(b"Make", b"HOND")
    ctx.serialize()
    ctx.find_path(b"Color")
    scol = ctx.extract_path_strings((b"Latitude",), cvt=True)
    lcol = ctx.extract_path_list((b"Make",), I)
    for c, (path, kind) in enumerate(columns):
        same_column(kind, ctx.fetch_table_column(c, nr, kind, nb[c]), want[c], ("after the other products", c))
    snr, snb = ctx.extract_path_strings((b"Latitude",), cvt=True, fetch=False)
    lnr, lne = ctx.extract_path_list((b"Make",), I, fetch=False)
    ctx.marshal_json(fetch=False)
    ctx.extract_table(columns[:2], fetch=False)
    same_column(SC, ctx.fetch_path_strings(snr, snb), scol, "the string column after a table")
    loff, lvals, lst = ctx.fetch_path_list(lnr, lne, I)
    assert np.array_equal(loff, lcol[0]) and np.array_equal(lst, lcol[2])
    tl = np.empty(len(text), dtype=np.uint8)
    ctx._check(sjhip.lib().sjhip_fetch_marshaled(ctx._h, tl.ctypes.data))
    assert tl.tobytes() == text
    # a second table replaces the first: no stale bytes, and the columns the first one had are gone
    ctx.parse(b'{"s":"a much longer string than the next","n":7}\n{"s":"b"}', ndjson=True)
    ctx.extract_table([((b"s",), S), ((b"n",), I), ((b"s",), SC)], fetch=False)
    (off, data, st), = ctx.extract_table([((b"n",), SC)])
    assert off.tolist() == [0, 1, 1] and data == b"7" and st.tolist() == [0, CW.COL_NOT_FOUND]
    with pytest.raises(sjhip.ParseError):
        ctx.fetch_table_column(1, 2, I)
