"""GPU: sjhip_marshal_rows_paths -- the selected rows projected onto k paths as NDJSON text -- against the serial restatement of
tests/project_rows_walk.py over the oracle's parse: text and offsets equal the model's at the seams of the row count (the write
kernel's 4 rows per block, the measure's 256, the scan's tile), of the column count and the plan's limits, of the cell size (one step
of the span walk, lane against wave, one long cell among short ones), of string values and name pieces, under every kind of
absence with and without SJHIP_PROJECT_NULLS, on every kind of row, on every number formatting branch, in every parse mode, composed
with the selecting calls and the other products, and in its errors."""
import json
import random

import numpy as np
import pytest

import marshal_rows_walk as MW
import number_cases as NC
import project_rows_walk as PW
import rows_walk as RW
from test_gpu_columns import oracle_walk
from test_gpu_marshal_rows import first_difference, raises_arg, sized_row
from test_gpu_parse import ctx  # noqa: F401
from test_gpu_tables import KINDS6, same_column

pytestmark = pytest.mark.gpu

F, I, U, B, S, SC = KINDS6
MR_SHORT = 128  # csrc/marshal.hip: the words of a cell its lane measures alone
MS_LONG = 64    # ... and the bytes from which a string, or a name piece, is handled by a whole wave


def check_project(ctx, w, rows, columns, names=None, nulls=False, what=None):
    """marshal_rows_paths on the selection in force -- whose row index is `rows` -- equals the restatement: text, n_rows, text_len
    and offsets; sjhip_fetch_marshaled delivers the same text; -> the device's text"""
    import sjhip
    text, offsets = PW.project_rows(w, rows, columns, names, nulls)
    assert ctx.marshal_rows_paths(columns, names, nulls, fetch=False) == (len(rows), len(text)), what
    n, got, off = ctx.marshal_rows_paths(columns, names, nulls, offsets=True)
    assert n == len(rows), what
    assert got == text, (what, first_difference(got, text))
    assert off.dtype == np.uint64 and off.tolist() == offsets, what
    out = np.zeros(len(text) + 1, np.uint8)
    assert sjhip.lib().sjhip_fetch_marshaled(ctx._h, out.ctypes.data) == 0
    assert out[:len(text)].tobytes() == text and out[len(text)] == 0, what
    return got


def array_doc(ctx, texts, copy=True, kf=True):
    """the rows are the elements of one array: parsed on both sides, selected -> (walk, row index)"""
    doc = ("[" + ",".join(texts) + "]").encode()
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy, key_flags=kf)
    rows = RW.select_rows(w, ())[1]
    assert ctx.select_rows(()) == (1, len(texts)) and len(rows) == len(texts)
    return w, rows


# ---- the seams of the row count ---------------------------------------------------------------------------------------------------
ROW_COUNTS = (0, 1, 4, 5, 255, 256, 257, 1025)


def count_rows(n):
    kinds = ['{"id":%d,"s":"t%d","o":{"k":[%d,null]}}', '{"s":"only s %d"}', "%d", '{"o":{"k":"%d"},"id":-%d.5}', '[{"id":%d}]']
    return [kinds[r % 5].replace("%d", str(r)) for r in range(n)]


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_at_the_seams(ctx, n):
    check_row_count(ctx, n)


def check_row_count(ctx, n):
    w, rows = array_doc(ctx, count_rows(n))
    for nulls in (False, True):
        text = check_project(ctx, w, rows, [(b"id",), (b"o", b"k"), (b"s",)], None, nulls, (n, nulls))
    if n >= 5:
        assert text.split(b"\n")[:5] == [b'{"id":0,"k":[0,null],"s":"t0"}', b'{"id":null,"k":null,"s":"only s 1"}',
                                         b'{"id":null,"k":null,"s":null}', b'{"id":-3.5,"k":"3","s":null}', b'{"id":null,"k":null,"s":null}']
    ctx.select_records()


# ---- the column count and the limits of a plan ------------------------------------------------------------------------------------
DEEP = [b"k%d" % j for j in range(16)]


def nested(keys, leaf):
    return "".join('{"%s":' % k.decode() for k in keys) + leaf + "}" * len(keys)


def test_one_column_sixteen_columns_and_the_limits_of_a_plan(ctx):
    deep = nested(DEEP, '"bottom"')[1:-1]  # the members of the row that holds the 16-key path
    texts = ['{%s,"p":{"q":%d},%s}' % (",".join('"c%d":%d' % (c, 100 * r + c) for c in range(14) if (r + c) % 5), r, deep) for r in range(9)] + \
            ['{"k0":{"k1":7}}', "{}"]
    w, rows = array_doc(ctx, texts)
    check_project(ctx, w, rows, [(b"c3",)], None, False, "one column")
    columns = [tuple(DEEP), (b"p", b"q")] + [(b"c%d" % c,) for c in range(14)]
    assert len(columns) == 16 and sum(len(p) for p in columns) == 32
    for nulls in (False, True):
        text = check_project(ctx, w, rows, columns, None, nulls, ("16 columns, 32 keys, a 16-key path", nulls))
    assert text.split(b"\n")[-2:] == [b"{" + b",".join(b'"%s":null' % p[-1] for p in columns) + b"}"] * 2
    ctx.select_records()


# ---- cell sizes ---------------------------------------------------------------------------------------------------------------------
def check_cell_sizes(ctx):
    """cells of 63 / 64 / 65 words (one step of the span walk) and 127 / 128 / 129 (a lane against the wave), alone and beside a
    second cell; one cell of several thousand words beside one-word cells in the same wave"""
    texts = []
    for words in (63, 64, 65, 127, 128, 129):
        ones = 1 if words % 2 else 2
        texts.append('{"c":%s,"x":true}' % sized_row(words, ones, words))
        texts.append('{"x":null,"c":{"in":%s}}' % sized_row(words - 4, ones, words + 1))
    big = len(texts)
    texts.append('{"x":false,"c":%s}' % sized_row(5002, 0, 3))
    texts += ['{"c":%d,"x":true}' % r for r in range(20)]
    w, rows = array_doc(ctx, texts)
    cells = [PW.indexes(w, v, [(b"c",)])[0] for v in rows]
    assert [MW.row_end(w, x) - x for x in cells[:big + 1]] == [63, 63, 64, 64, 65, 65, 127, 127, 128, 128, 129, 129, 5002]
    check_project(ctx, w, rows, [(b"c",), (b"x",)], None, False, "cell sizes")
    check_project(ctx, w, rows, [(b"x",), (b"c",), (b"c",)], [b"x", b"c", b"again"], True, "cell sizes, twice")
    ctx.select_records()


def test_cell_sizes_at_the_seams(ctx):
    check_cell_sizes(ctx)


# ---- string values --------------------------------------------------------------------------------------------------------------------
STRING_LENGTHS = (0, 7, 8, 63, 64, 65, 511, 512, 513)
ESCAPES = '"\\\n\t\b\f\r\x01\x1f'


def string_values():
    """strings of the seam lengths: plain; with bytes that escape, spread and at both ends"""
    out = []
    for n in STRING_LENGTHS:
        plain = ("abcdefghijklmnopqrstuvwxyz" * 20)[:n]
        out.append(plain)
        if n:
            out.append((ESCAPES * 60)[:n])
            out.append('"' + plain[1:n - 1] + ("\x01" if n > 1 else ""))
    return out


def check_strings(ctx, copy, kf):
    values = string_values()
    texts = ['{"s":%s,"n":%d}' % (json.dumps(s), k) for k, s in enumerate(values)]
    w, rows = array_doc(ctx, texts, copy, kf)
    text = check_project(ctx, w, rows, [(b"s",), (b"n",)], None, False, ("strings", copy, kf))
    assert [json.loads(l)["s"] for l in text.split(b"\n")] == values
    ctx.select_records()


def test_string_values_at_the_seams(ctx):
    check_strings(ctx, True, True)


# ---- name pieces ----------------------------------------------------------------------------------------------------------------------
def seam_names():
    """names whose escaped piece -- '"' + escapeBytes(name) + '":' -- is 3 (the empty name), 63, 64, 65 and 513 bytes long, plain and
    with escapes; names of quotes, backslashes, every control byte, multi-byte UTF-8, U+2028 and U+2029"""
    names = [b""]
    for piece in (63, 64, 65, 513):
        names.append((b"name" * 200)[:piece - 3])
        units = (piece - 7) // 10  # '\\' and '"' escape to 4 bytes, every unit of 4 to 10, a 'p' to itself
        names.append(b'\\"' + b"n\x01m\n" * units + b"p" * (piece - 7 - 10 * units))
    names += [b'"', b"\\", b'q"\\"', bytes(range(0x20)), "é中\U0001f600".encode(), "a b c".encode()]
    return names


def check_names(ctx):
    names = seam_names()
    pieces = [len(PW.name_text(x)) + 1 for x in names]
    assert pieces[0] == 3 and {63, 64, 65, 513} <= set(pieces), pieces
    texts = ['{"a":%d,"b":"v%d"}' % (r, r) for r in range(6)] + ['{"b":[]}', "{}"]
    w, rows = array_doc(ctx, texts)
    for k in range(0, len(names), 2):  # (two at a time: the names of one call hold at most 1024 bytes)
        mine = names[k:k + 2]
        columns = [(b"a",), (b"b",)][:len(mine)]
        for nulls in (False, True):
            check_project(ctx, w, rows, columns, mine, nulls, ("names", k, nulls))
    # repeated names, the same long one twice, and all of a name budget: 1024 bytes in 16 names
    text = check_project(ctx, w, rows, [(b"a",), (b"b",), (b"a",)], [b"x", b"x", b"x"], False, "repeated names")
    assert text.split(b"\n")[0] == b'{"x":0,"x":"v0","x":0}'
    check_project(ctx, w, rows, [(b"a",), (b"b",)], [names[7], names[7]], True, "a long name twice")
    check_project(ctx, w, rows, [(b"a",), (b"b",)] * 8, [b"\x02" * 64] * 16, True, "1024 name bytes, all escaped")
    ctx.select_records()


def test_name_pieces_at_the_seams(ctx):
    check_names(ctx)


# ---- absence --------------------------------------------------------------------------------------------------------------------------
def check_absence(ctx):
    texts = []
    for r in range(70):  # more than one wave
        texts.append(['{"m":%d,"z":"last"}', '{"a":"first","m":%d}', '{"other":%d}', '{"a":1,"m":%d,"z":2}'][r % 4] % r if r % 2 or r < 40 else '{"q":%d}' % r)
    texts += ['{"a":5,"a":{"b":"second a"},"m":1}',       # NOT_OBJECT on the way: a.b where the first a is a number; the first key wins
              '{"a":{"b":null},"m":null,"z":null}',        # a present null
              '{"a":{"b":"first"},"a":{"b":"second"},"m":"one","m":"two"}',
              '"scalar"', "[1,2]", "null"]
    w, rows = array_doc(ctx, texts)
    for nulls in (False, True):
        text = check_project(ctx, w, rows, [(b"a",), (b"m",), (b"z",)], None, nulls, ("first, last, all absent", nulls))
        tail = check_project(ctx, w, rows, [(b"a", b"b"), (b"m",)], [b"ab", b"m"], nulls, ("NOT_OBJECT, null, duplicates", nulls)).split(b"\n")[70:]
    lines = text.split(b"\n")
    assert lines[0] == b'{"a":null,"m":0,"z":"last"}' and lines[1] == b'{"a":"first","m":1,"z":null}' and lines[2] == b'{"a":null,"m":null,"z":null}'
    assert tail == [b'{"ab":null,"m":1}', b'{"ab":null,"m":null}', b'{"ab":"first","m":"one"}'] + [b'{"ab":null,"m":null}'] * 3
    lines = check_project(ctx, w, rows, [(b"a",), (b"m",), (b"z",)], None, False).split(b"\n")
    assert lines[:4] == [b'{"m":0,"z":"last"}', b'{"a":"first","m":1}', b"{}", b'{"a":1,"m":3,"z":2}'] and lines[-1] == b"{}"
    assert check_project(ctx, w, rows, [(b"nowhere",), (b"a", b"b", b"c")], None, False) == b"\n".join([b"{}"] * len(rows))
    ctx.select_records()


def test_absent_columns_with_and_without_nulls(ctx):
    check_absence(ctx)


# ---- row kinds --------------------------------------------------------------------------------------------------------------------------
def test_row_kinds_prefix_paths_and_one_path_twice(ctx):
    texts = ['"a string"', '""', "12", "-0.5", "1e21", "true", "false", "null",
             '{"user":{"name":"N","id":7},"id":1}', '{"user":"not an object","id":2}', '{"user":{"id":3}}', "{}",
             '[{"user":{"name":"in an array"}},2]', "[]", '{"user":{"name":{"first":"F"}}}']
    w, rows = array_doc(ctx, texts)
    for nulls in (False, True):
        text = check_project(ctx, w, rows, [(), (b"user",), (b"user", b"name"), (b"id",), (b"user",), ()],
                             [b"row", b"user", b"name", b"id", b"user too", b"row too"], nulls, ("row kinds", nulls))
    lines = text.split(b"\n")
    assert lines[0] == b'{"row":"a string","user":null,"name":null,"id":null,"user too":null,"row too":"a string"}'
    assert lines[8] == b'{"row":%s,"user":{"name":"N","id":7},"name":"N","id":1,"user too":{"name":"N","id":7},"row too":%s}' % ((texts[8].encode(),) * 2)
    assert lines[9] == b'{"row":%s,"user":"not an object","name":null,"id":2,"user too":"not an object","row too":%s}' % ((texts[9].encode(),) * 2)
    assert check_project(ctx, w, rows, [()], [b""], False, "only the row").split(b"\n")[:3] == [b'{"":"a string"}', b'{"":""}', b'{"":12}']
    ctx.select_records()


# ---- numbers --------------------------------------------------------------------------------------------------------------------------
def test_numbers_as_cells(ctx):
    named = ["-0.0", "1e20", "1e21", "9223372036854775807", "-9223372036854775808", "9223372036854775808", "18446744073709551615",
             "0.000001", "1e-7", "5e-324", "1.7976931348623157e308", "0", "-1", "1E+2"]
    sample = NC.sample(random.Random(33), 600)
    values = named + sample
    texts = ['{"v":%s,"w":[%s]}' % (x, values[(k + 1) % len(values)]) for k, x in enumerate(values)] + \
            ['{"v":[%s]}' % ",".join(sample)]  # ... and all of them in one cell that the wave walks
    w, rows = array_doc(ctx, texts)
    text = check_project(ctx, w, rows, [(b"v",), (b"w",)], None, False, "numbers")
    assert text.split(b"\n")[:3] == [b'{"v":-0,"w":[100000000000000000000]}', b'{"v":100000000000000000000,"w":[1e+21]}',
                                     b'{"v":1e+21,"w":[9223372036854775807]}']
    ctx.select_records()


# ---- parse modes ----------------------------------------------------------------------------------------------------------------------
def check_parse_mode(ctx, copy, kf):
    """containers as cells: ':' behind keys and ',' behind values inside them, strings with escapes (copied or read from the message)"""
    texts = ['{"o":{"k%d":"k%d","e\\n":["k%d",{"k%d":{"x":"y\\t"}},"%s"],"z":{}},"a":["s",{"s":"s"},[]],"s":"plain %d"}' %
             (r, r, r, r, "l" * (60 + r), r) for r in range(9)]
    w, rows = array_doc(ctx, texts, copy, kf)
    text = check_project(ctx, w, rows, [(b"o",), (b"a",), (b"o", b"e\n"), (b"s",)], None, True, ("parse mode", copy, kf))
    assert [json.loads(l) for l in text.split(b"\n")] == [dict(o=t["o"], a=t["a"], s=t["s"], **{"e\n": t["o"]["e\n"]}) for t in map(json.loads, texts)]
    ctx.select_records()
    return text


def test_parse_modes(ctx):
    got = {check_parse_mode(ctx, copy, kf) for copy in (True, False) for kf in (True, False)}
    assert len(got) == 1
    check_strings(ctx, False, False)


# ---- composition ------------------------------------------------------------------------------------------------------------------------
COLUMNS = [(b"id",), (b"u", b"n"), (b"tags",)]


def nd_doc():
    recs = []
    for k in range(12):
        items = ['{"id":%d,"u":{"n":"user %d"},"tags":[%s],"score":%d}' % (10 * k + j, j, ",".join('"t%d"' % t for t in range(j)), (7 * k + 3 * j) % 11)
                 for j in range(k % 4)]
        recs.append('{"rec":%d,"items":[%s]}' % (k, ",".join(items)))
    return "\n".join(recs).encode()


def device_rows(ctx, records, rows):
    return [int(x) for x in ctx.fetch_rows(records, rows)[1]]


def test_composition_with_the_selecting_calls(ctx):
    doc = nd_doc()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    # after select_rows
    nr, n = ctx.select_rows((b"items",))
    rows = RW.select_rows(w, (b"items",))[1]
    assert device_rows(ctx, nr, n) == rows and n == 18
    check_project(ctx, w, rows, COLUMNS, None, True, "after select_rows")
    # after order_path with a limit
    o = ctx.order_path((b"score",), I, descending=True, limit=5)
    kept = device_rows(ctx, o.records, o.rows)
    assert o.rows == 5 and set(kept) < set(rows)
    check_project(ctx, w, kept, COLUMNS, None, False, "after order_path")
    ctx.select_records()
    # after where_path without a selection: the records are the rows
    nr, n = ctx.where_path((b"rec",), ctx.OP_GE_INT, 4)
    kept = device_rows(ctx, nr, n)
    assert n == 8 and kept == [r + 1 for r in w.records()][4:]
    text = check_project(ctx, w, kept, [(b"rec",), (b"items",)], [b"r", b"items"], False, "after where_path")
    assert text.split(b"\n")[0] == b'{"r":4,"items":[]}'
    # after unnest_rows
    nr, npar, n = ctx.unnest_rows((b"items",))
    kept = device_rows(ctx, nr, n)
    assert npar == 8 and n == 12
    check_project(ctx, w, kept, COLUMNS + [()], [b"id", b"n", b"tags", b"row"], True, "after unnest_rows")
    ctx.select_records()


def test_composition_with_the_other_products(ctx):
    doc = nd_doc()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    nr, n = ctx.select_rows((b"items",))
    rows = RW.select_rows(w, (b"items",))[1]
    selection = ctx.fetch_rows(nr, n)
    tnr, tnb = ctx.extract_table([((b"u", b"n"), S), ((b"id",), I)], fetch=False)
    tcols = [ctx.fetch_table_column(0, tnr, S, tnb[0]), ctx.fetch_table_column(1, tnr, I)]
    text = check_project(ctx, w, rows, COLUMNS, None, False, "under the table")
    # the table extracted before the call fetches unchanged after it, and so does the selection
    same_column(S, ctx.fetch_table_column(0, tnr, S, tnb[0]), tcols[0], "the table's string column after marshal_rows_paths")
    same_column(I, ctx.fetch_table_column(1, tnr, I), tcols[1], "the table's int column after marshal_rows_paths")
    for a, b in zip(ctx.fetch_rows(nr, n), selection):
        assert np.array_equal(a, b)
    # marshal_rows after it gives its usual bytes, and the projection after that its own again
    whole, offsets = MW.marshal_rows(w, rows)
    n2, got, off = ctx.marshal_rows(offsets=True)
    assert (n2, got, off.tolist()) == (len(rows), whole, offsets)
    assert ctx.marshal_rows_paths(COLUMNS) == (len(rows), text)
    assert ctx.marshal_json() == doc
    ctx.select_records()


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
def test_errors_touch_nothing(ctx):
    import ctypes as C

    import sjhip
    L = sjhip.lib()
    fresh = sjhip.Context(0)
    raises_arg(lambda: fresh.marshal_rows_paths([(b"a",)]))  # no result at all
    doc = b'{"k":"v","items":[{"a":"x"},{"a":"y","b":1}]}\n{"k":"w","items":[{"a":"z"},7]}'
    fresh.parse(doc, ndjson=True)
    whole = fresh.marshal_json()
    raises_arg(lambda: fresh.marshal_rows_paths([(b"a",)]), "no row selection")
    out = np.empty(len(whole), np.uint8)
    assert L.sjhip_fetch_marshaled(fresh._h, out.ctypes.data) == 0 and out.tobytes() == whole  # (the text of marshal_json is still there)
    nr, n = fresh.select_rows((b"items",))
    selection = fresh.fetch_rows(nr, n)
    before = fresh.marshal_rows_paths([(b"a",)], offsets=True)
    assert before[:2] == (4, b'{"a":"x"}\n{"a":"y"}\n{"a":"z"}\n{}') and before[2].tolist() == [0, 10, 20, 30, 33]

    def intact():
        got = np.zeros(len(before[1]), np.uint8)
        off = np.zeros(5, np.uint64)
        assert L.sjhip_fetch_marshaled_rows(fresh._h, off.ctypes.data, got.ctypes.data) == 0
        assert got.tobytes() == before[1] and off.tolist() == before[2].tolist()
        for a, b in zip(fresh.fetch_rows(nr, n), selection):
            assert np.array_equal(a, b)

    u32 = lambda *xs: (C.c_uint32 * len(xs))(*xs)  # noqa: E731
    n_out, tl = C.c_uint64(0), C.c_size_t(0)

    def call(keys, key_lens, path_lens, n_cols, names, name_lens, flags):
        return fresh._check(L.sjhip_marshal_rows_paths(fresh._h, keys, key_lens, path_lens, n_cols, names, name_lens, flags, C.byref(n_out), C.byref(tl)))

    key17 = [(b"k",) * 17]
    cases = [
        (lambda: call(b"a", u32(1), u32(1), 1, None, None, 2), ("unknown flag",)),
        (lambda: call(b"a", u32(1), u32(1), 1, None, None, 0x80000001), ("unknown flag",)),
        (lambda: call(b"a", u32(1), u32(1), 0, None, None, 0), ("0 columns", "1 to 16")),
        (lambda: fresh.marshal_rows_paths([(b"a",)] * 17), ("17 columns", "1 to 16")),
        (lambda: fresh.marshal_rows_paths(key17), ("column 0", "more than 16 keys")),
        (lambda: fresh.marshal_rows_paths([(b"a",)] + [(b"k",) * 16, (b"j",) * 16]), ("column 2", "more than 32 keys")),
        (lambda: fresh.marshal_rows_paths([(b"a",), (b"x" * 1024,)]), ("column 1", "longer than 1024 bytes")),
        (lambda: fresh.marshal_rows_paths([(b"a",), (b"b",)], [b"n" * 1000, b"m" * 25]), ("column 1", "names", "1024 bytes")),
        (lambda: fresh.marshal_rows_paths([(b"a",), ()]), ("column 1", "empty path")),
    ]
    for attempt, texts in cases:
        raises_arg(attempt, *texts)
        intact()
    # the limits themselves are legal
    assert fresh.marshal_rows_paths([(b"a",), ()], [b"n" * 1000, b"m" * 24], fetch=False)[0] == 4
    assert fresh.marshal_rows_paths([(b"a",)], nulls=True) == (4, b'{"a":"x"}\n{"a":"y"}\n{"a":"z"}\n{"a":null}')
    fresh.close()


def test_sharded_result_is_refused(ctx):
    """in sjhip_marshal_rows' words, and the selection stays in force"""
    import fixtures
    import sjhip
    line = b'{"items":[{"a":"' + b"x" * 200 + b'"}]}'
    big = b"\n".join([line] * (3 * (1 << 20) // len(line)))
    with fixtures.nd_shard_limits(2 << 20, 1 << 20):
        many = sjhip.Context(0)
        many.parse(big, ndjson=True)
    rows = many.select_rows((b"items",))[1]
    assert rows > 1000
    wording = []
    for call, name in ((lambda: many.marshal_rows_paths([(b"a",)]), "sjhip_marshal_rows_paths"), (many.marshal_rows, "sjhip_marshal_rows")):
        raises_arg(call, name + " works on the result of one context", "shard by shard")
        wording.append(many.last_error().replace(name, "CALL"))
    assert wording[0] == wording[1]
    assert len(many.find_path(b"a")) == rows  # (the selection is still in force)
    many.close()
