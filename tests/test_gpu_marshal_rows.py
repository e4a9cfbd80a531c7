"""GPU: sjhip_marshal_rows -- the selected rows as NDJSON text -- against the serial restatement of tests/marshal_rows_walk.py over
the oracle's parse (the oracle's own formatter, row by row), and against the oracle's MarshalJSON where whole documents are known:
parity under select_rows and where_path, the seams of the row count (the wave-per-row blocks of 4, the wave, the block, the
1024-row scan tile) and of the row length (the 64-word step, the lane / wave threshold, one long row), raw words that look like
tags, strings of every length and content as keys and values with and without copied strings and parser key flags, numbers,
equivalence with sjhip_marshal_json, the fixtures, errors and the lifecycle."""
import json
import random

import numpy as np
import pytest

import fixtures
import marshal_rows_walk as MW
import number_cases as NC
import oracle_lib as O
import query_walk as Q
import rows_walk as RW
import where_walk as WW
from test_filter_rows_walk import items_doc, kinds_rows
from test_gpu_columns import oracle_walk
from test_gpu_parse import ctx  # noqa: F401
from test_gpu_rows import RAW
from test_gpu_tables import KINDS6, same_column

pytestmark = pytest.mark.gpu

F, I, U, B, S, SC = KINDS6
MR_SHORT = 128  # csrc/marshal.hip: the words of a row its lane measures alone; a longer row is measured by its wave
MS_LONG = 64    # ... and the bytes from which a string is measured and written by a whole wave


def check_marshal(ctx, w, rows, what=None):
    """marshal_rows on the selection in force -- whose row index is `rows` -- equals the restatement: text, n_rows, text_len and
    offsets; sjhip_fetch_marshaled delivers the same text; -> the device's text"""
    import sjhip
    text, offsets = MW.marshal_rows(w, rows)
    assert ctx.marshal_rows(fetch=False) == (len(rows), len(text)), what
    n, got, off = ctx.marshal_rows(offsets=True)
    assert n == len(rows), what
    assert got == text, (what, first_difference(got, text))
    assert off.dtype == np.uint64 and off.tolist() == offsets, what
    out = np.zeros(len(text) + 1, np.uint8)
    assert sjhip.lib().sjhip_fetch_marshaled(ctx._h, out.ctypes.data) == 0
    assert out[:len(text)].tobytes() == text and out[len(text)] == 0, what
    assert ctx.marshal_rows() == (n, text), what
    return got


def first_difference(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return k, len(a), len(b), a[max(0, k - 30):k + 30], b[max(0, k - 30):k + 30]


# ---- parity -----------------------------------------------------------------------------------------------------------------------
def test_parity_on_items(ctx):
    doc, order, box = items_doc(kinds_rows(150), scalars_every=9)
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    sel = RW.select_rows(w, (b"items",))
    all_rows = sel[1]
    assert ctx.select_rows((b"items",))[1] == len(all_rows) == len(order) and box.count(False) > 5
    text = check_marshal(ctx, w, all_rows, "every row")
    assert [json.loads(l) for l in text.split(b"\n")] == [json.loads(t) for t in order]
    for negate in (False, True):
        ctx.select_rows((b"items",))
        kept = WW.where(w, sel, (b"r",), WW.OP_GE_INT, 40, negate)
        assert ctx.where_path((b"r",), ctx.OP_GE_INT, 40, negate=negate)[1] == len(kept[1]) > 0
        check_marshal(ctx, w, kept[1], ("r >= 40", negate))
    ctx.select_rows((b"items",))
    kept = WW.where(w, sel, (b"r",), WW.OP_GE_INT, 40, False)
    kept = WW.where(w, kept, (b"w",), WW.OP_PREFIX_STRING, b"row 1", False)  # two successive calls: the conjunction
    ctx.where_path((b"r",), ctx.OP_GE_INT, 40)
    assert ctx.where_path((b"w",), ctx.OP_PREFIX_STRING, b"row 1")[1] == len(kept[1]) > 0
    check_marshal(ctx, w, kept[1], "r >= 40 and w has the prefix")
    ctx.select_records()


# ---- the seams of the row count ---------------------------------------------------------------------------------------------------
ROW_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
SCALARS = ['"s%d"', "%d", "-%d.5", "true", "null"]


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_at_the_seams(ctx, n):
    texts = [('{"v":%d,"s":"%s"}' % (r, "t" * (r % 7) + str(r)) if r % 5 else '[%d,{"a":1}]' % r) if r % 3 else
             (SCALARS[r % 5] % r if "%" in SCALARS[r % 5] else SCALARS[r % 5]) for r in range(n)]
    doc = ("[" + ",".join(texts) + "]").encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rows = RW.select_rows(w, ())[1]
    assert ctx.select_rows(()) == (1, n) and len(rows) == n
    text = check_marshal(ctx, w, rows, n)
    assert text == "\n".join(texts).encode()  # (the texts are compact as they stand)
    ctx.select_records()


# ---- the seams of the row length, and raw words that look like tags -------------------------------------------------------------
# integers whose value word has the top byte { [ } ] " l u d t f n r
RAWS = list(RAW.values()) + [(ord(c) << 56) + 12345 + k for k, c in enumerate("udtfnr")]


def sized_row(words, ones, seed=0):
    """an array row of exactly `words` tape words: [ , `ones` one-word atoms, two-word entries, ] -- the two-word entries are
    integers whose value words look like tags and strings: every third entry, and every entry whose tag word is the last word of
    a 64-word step (its length word lies in the next step).  With ones even the two-word entries start at odd indices, so one
    of them straddles every step."""
    twos = words - 2 - ones
    assert twos >= 4 and twos % 2 == 0
    items = []
    for k in range(twos // 2):
        at = 1 + ones + 2 * k
        if at % 64 == 63 or k % 3 == 0:
            items.append('"%s"' % ("s%d\\n" % at * (1 + k % 4)))
        else:
            items.append(str(RAWS[(seed + k) % len(RAWS)]))
    return "[" + ",".join(["true", "null", "false"][:ones] + items) + "]"


ROW_LENGTHS = list(range(62, 67)) + list(range(126, 131))


def check_row_lengths(ctx):
    texts, lengths = [], []
    for k, words in enumerate(ROW_LENGTHS):
        for ones in ((0, 2) if words % 2 == 0 else (1, 3)):
            row = sized_row(words, ones, k)
            if (k + ones) % 4 == 3:  # ... and some as the value of an object's member: four words more
                row = '{"k%d":%s}' % (words, sized_row(words - 4, ones, k))
            texts.append(row)
            lengths.append(words)
    assert any('"s63' in t for t in texts) and any('"s127' in t for t in texts)
    doc = ("[" + ",".join(texts) + "]").encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rows = RW.select_rows(w, ())[1]
    assert [(w.t[v] & Q.MASK) - v for v in rows] == lengths  # every row is as long as it was meant to be
    assert ctx.select_rows(())[1] == len(rows)
    assert check_marshal(ctx, w, rows, "row lengths") == "\n".join(texts).encode()
    key = sorted(t[2:t.index('"', 2)] for t in texts if t[0] == "{")[0].encode()  # ... and with the rows that have this key dropped
    sel = WW.where(w, RW.select_rows(w, ()), (key,), Q.OP_EXISTS, None, True)
    ctx.where_path((key,), ctx.OP_EXISTS, negate=True)
    assert 0 < len(sel[1]) < len(rows)
    check_marshal(ctx, w, sel[1], "row lengths, narrowed")
    ctx.select_records()


def test_row_lengths_at_the_seams(ctx):
    check_row_lengths(ctx)


def check_one_long_row(ctx):
    """one row of about 5 000 words among two-word rows: the wave walks it while the other lanes of its wave are done"""
    big = sized_row(5002, 0, 3)
    texts = ["[]", "{}", '"x"', big, "[]", "7", '{"a":"after"}', "{}"]
    doc = ("[" + ",".join(texts) + "]").encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rows = RW.select_rows(w, ())[1]
    assert (w.t[rows[3]] & Q.MASK) - rows[3] == 5002
    ctx.select_rows(())
    assert check_marshal(ctx, w, rows, "one long row") == "\n".join(texts).encode()
    ctx.select_records()


def test_one_long_row_between_short_ones(ctx):
    check_one_long_row(ctx)


# ---- strings ------------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 200)
ESCAPES = '"\\\n\t\b\f\r\x01\x1f'


def string_cases():
    """strings of every length (in bytes): plain, made only of escapes, with an escape exactly in front of and behind the 8-byte
    and the 64-byte seam, with multi-byte UTF-8"""
    out = []
    for n in LENGTHS:
        plain = ("abcdefghijklmnopqrstuvwxyz" * 8)[:n]
        out.append(plain)
        out.append((ESCAPES * 23)[:n])
        for at, c in ((7, '"'), (8, "\\"), (63, "\n"), (64, "\x01"), (n - 1, "\x1f"), (0, "\t")):
            if 0 <= at < n:
                out.append(plain[:at] + c + plain[at + 1:])
        if n >= 9:
            multi = "é中\U0001f600"  # 2 + 3 + 4 bytes
            out.append(multi + plain[:n - 9])
            out.append(plain[:n - 9] + multi)
    return out


def strings_doc():
    texts = []
    for s in string_cases():
        q = json.dumps(s, ensure_ascii=False)
        texts += ["{%s:%s}" % (q, q), q, "[%s,{%s:[%s]}]" % (q, q, q)]  # as key and value (a value equal to its key), as a scalar row, nested
    return ("[" + ",".join(texts) + "]").encode("utf-8"), texts


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
@pytest.mark.parametrize("kf", [True, False], ids=["parser key flags", "recovered key flags"])
def test_strings_as_keys_and_values(ctx, copy, kf):
    check_strings(ctx, copy, kf)


def check_strings(ctx, copy, kf):
    doc, texts = strings_doc()
    w = oracle_walk(doc, False, copy)
    ctx.parse(doc, copy_strings=copy, key_flags=kf)
    rows = RW.select_rows(w, ())[1]
    assert ctx.select_rows(())[1] == len(rows) == len(texts)
    text = check_marshal(ctx, w, rows, ("strings", copy, kf))
    assert [json.loads(l) for l in text.split(b"\n")] == [json.loads(t) for t in texts]
    ctx.select_records()


# ---- keys and values ----------------------------------------------------------------------------------------------------------------
SHAPES = ['{"a":{"b":[{"c":{"d":[{"e":"f"}]}}]}}', "{}", "[]", '{"":""}', '{"":{"":[]},"x":{}}', '[[],{},[[]],[{}]]', '{"k":"k","v":["k","v"]}',
          '[{"a":"a"},"a",{"a":["a",{"a":"a"}]}]', '{"t":true,"f":false,"n":null,"l":-1,"u":18446744073709551615,"d":0.5}', '""', '"k"']


def test_keys_and_values_with_and_without_parser_flags(ctx):
    texts = SHAPES * 3
    doc = ("\n".join('{"items":[%s]}' % ",".join(texts[k:k + 4]) for k in range(0, len(texts), 4))).encode()
    w = oracle_walk(doc, True, True)
    got = []
    for kf in (True, False):
        ctx.parse(doc, ndjson=True, key_flags=kf)
        rows = RW.select_rows(w, (b"items",))[1]
        assert ctx.select_rows((b"items",))[1] == len(rows) == len(texts)
        got.append(check_marshal(ctx, w, rows, ("shapes", kf)))
        ctx.select_records()
    assert got[0] == got[1] == "\n".join(texts).encode()


def test_recovered_key_flags_on_a_long_tape(ctx):
    """without the parser's flags the per-tape-index array is built over the whole tape, 2048 words per tile: several tiles, strings
    at the tile seams, and a run of raw words that look like string tags in front of a tile (the anchor is searched further back)"""
    run = ",".join([str(RAW['"'])] * 2100)  # 4200 words of l-entries whose value word looks like a string tag
    texts = ['{"k%d":"v%d","n":[%d,"s"]}' % (r, r, r) for r in range(700)] + ['{"run":[%s],"after":"x"}' % run] + \
            ['{"z%d":{"z":"z"}}' % r for r in range(300)]
    doc = ("[" + ",".join(texts) + "]").encode()
    w = oracle_walk(doc, False, True)
    assert len(w.t) > 5 * 2048
    got = []
    for kf in (False, True):
        ctx.parse(doc, key_flags=kf)
        ctx.select_rows(())
        ctx.where_path((b"n", ), ctx.OP_EXISTS, negate=True)  # the rows behind the tile seams
        sel = WW.where(w, RW.select_rows(w, ()), (b"n",), Q.OP_EXISTS, None, True)
        assert len(sel[1]) == 301
        got.append(check_marshal(ctx, w, sel[1], ("long tape", kf)))
        ctx.select_rows(())
        n, text = ctx.marshal_rows()
        assert n == 1001 and text == "\n".join(texts).encode()
        assert ctx.marshal_json() == doc  # (MarshalJSON afterwards is what it is without the call)
        ctx.select_records()
    assert got[0] == got[1]


# ---- numbers ------------------------------------------------------------------------------------------------------------------------
def test_numbers(ctx):
    named = ["-0.0", "1e20", "1e21", "9223372036854775807", "-9223372036854775808", "9223372036854775808", "18446744073709551615",
             "0.000001", "1e-7", "5e-324", "1.7976931348623157e308", "0", "-1", "1E+2"]
    sample = NC.sample(random.Random(16), 3000)
    texts = ["[%s]" % ",".join(named), "[%s]" % ",".join(sample[:40]), "[%s]" % ",".join(sample)] + named  # lane, lane, wave, scalars
    doc = ("[" + ",".join(texts) + "]").encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rows = RW.select_rows(w, ())[1]
    assert ctx.select_rows(())[1] == len(rows) == len(texts)
    text = check_marshal(ctx, w, rows, "numbers")
    lines = text.split(b"\n")
    assert lines[0] == b"[-0,100000000000000000000,1e+21,9223372036854775807,-9223372036854775808,9223372036854775808," \
                       b"18446744073709551615,0.000001,1e-7,5e-324,1.7976931348623157e+308,0,-1,100]"
    assert lines[3:6] == [b"-0", b"100000000000000000000", b"1e+21"]
    ctx.select_records()


# ---- equivalence with MarshalJSON ---------------------------------------------------------------------------------------------------
def test_equals_marshal_json_on_parking(ctx):
    doc = fixtures.load("parking-citations") * 3
    ctx.parse(doc, ndjson=True, key_flags=True)
    whole = ctx.marshal_json()
    ref = O.parse(doc, ndjson=True)
    rc, want = O.marshal_json(ref.tape, ref.strings, doc)
    assert rc == 0 and whole == want
    records, rows = ctx.where_path((), ctx.OP_EXISTS)
    n, text, off = ctx.marshal_rows(offsets=True)
    assert n == rows == records and text == whole
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    assert np.array_equal(off[1:-1], nl + 1) and off[0] == 0 and off[-1] == len(text) + 1
    ctx.select_records()
    # Make == "HOND": the oracle's MarshalJSON of what the oracle-checked filter returns
    kept = ctx.where_path((b"Make",), ctx.OP_EQ_STRING, b"HOND")[1]
    n, text = ctx.marshal_rows()
    count, sub = ctx.filter_where(b"Make", b"HOND")
    assert n == kept == count == 348
    rc, want = O.marshal_json(sub.Tape, sub.Strings, b"")
    assert rc == 0 and text == want
    ctx.select_records()


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def test_twitter_statuses(ctx):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = RW.select_rows(w, (b"statuses",))
    ctx.select_rows((b"statuses",))
    kept = WW.where(w, sel, (b"retweet_count",), WW.OP_GE_INT, 10, False)
    assert ctx.where_path((b"retweet_count",), ctx.OP_GE_INT, 10)[1] == len(kept[1])
    want = [s for s in json.loads(doc)["statuses"] if s["retweet_count"] >= 10]
    assert 0 < len(want) == len(kept[1]) < 100
    text = check_marshal(ctx, w, kept[1], "retweet_count >= 10")
    assert [json.loads(l) for l in text.split(b"\n")] == want
    ctx.select_records()


def test_canada_rings(ctx):
    """the coordinate rings of canada.json -- arrays of arrays of numbers, no string at all -- as the rows"""
    doc = fixtures.load("canada")
    start = doc.index(b'"coordinates":') + len(b'"coordinates":')
    end = doc.rindex(b"]", 0, doc.rindex(b"]"))
    rings = json.loads(doc[start:end + 1])[:60]
    doc = json.dumps({"coordinates": rings}).encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rows = RW.select_rows(w, (b"coordinates",))[1]
    assert ctx.select_rows((b"coordinates",))[1] == len(rows) == 60
    text = check_marshal(ctx, w, rows, "rings")
    assert [json.loads(l) for l in text.split(b"\n")] == rings and b'"' not in text
    ctx.select_records()


# ---- errors and the lifecycle -------------------------------------------------------------------------------------------------------
def raises_arg(call, *texts):
    import sjhip
    with pytest.raises(sjhip.ParseError) as e:
        call()
    assert e.value.code == 5 and all(t in str(e.value) for t in texts), str(e.value)


def test_errors(ctx):
    import sjhip
    L = sjhip.lib()
    fresh = sjhip.Context(0)
    raises_arg(fresh.marshal_rows)  # no result at all
    raises_arg(lambda: fresh._check(L.sjhip_fetch_marshaled_rows(fresh._h, None, None)), "sjhip_marshal_rows")
    doc = b'{"k":"v","items":[{"a":"x"},{"a":"y"}]}\n{"k":"w","items":[{"a":"z"},7]}'
    # no selection; the refused call touches no product: the text of sjhip_marshal_json is still there
    fresh.parse(doc, ndjson=True)
    whole = fresh.marshal_json()
    assert whole == doc
    raises_arg(fresh.marshal_rows, "no row selection")
    out = np.empty(len(whole), np.uint8)
    assert L.sjhip_fetch_marshaled(fresh._h, out.ctypes.data) == 0 and out.tobytes() == whole
    # the text of sjhip_marshal_json has no rows
    off = np.zeros(8, np.uint64)
    raises_arg(lambda: fresh._check(L.sjhip_fetch_marshaled_rows(fresh._h, off.ctypes.data, out.ctypes.data)), "sjhip_marshal_json", "no rows")
    # either destination of the fetch, and either count of the call, may be null
    fresh.select_rows((b"items",))
    assert L.sjhip_marshal_rows(fresh._h, None, None) == 0
    assert L.sjhip_fetch_marshaled_rows(fresh._h, off.ctypes.data, None) == 0 and off[:5].tolist() == [0, 10, 20, 30, 32]
    text = np.zeros(31, np.uint8)
    assert L.sjhip_fetch_marshaled_rows(fresh._h, None, text.ctypes.data) == 0 and text.tobytes() == b'{"a":"x"}\n{"a":"y"}\n{"a":"z"}\n7'
    # no rows is legal
    assert fresh.where_path((b"nowhere",), fresh.OP_EXISTS)[1] == 0
    n, text, off = fresh.marshal_rows(offsets=True)
    assert (n, text, off.tolist()) == (0, b"", [0]) and fresh.marshal_rows(fetch=False) == (0, 0)
    fresh.close()


def test_lifecycle(ctx):
    import sjhip
    L = sjhip.lib()
    doc, order, box = items_doc(kinds_rows(90), scalars_every=11)
    w = oracle_walk(doc, True, True)
    for kf in (True, False):
        ctx.parse(doc, ndjson=True, key_flags=kf)
        whole = ctx.marshal_json()
        sel = RW.select_rows(w, (b"items",))
        nr, rows = ctx.select_rows((b"items",))
        kept = WW.where(w, sel, (b"r",), WW.OP_GE_INT, 30, False)
        nr, rows = ctx.where_path((b"r",), ctx.OP_GE_INT, 30)
        selection = ctx.fetch_rows(nr, rows)
        scol = ctx.extract_path_strings((b"w",), cvt=True)
        lcol = ctx.extract_path_list((b"v",), I)
        tnr, tnb = ctx.extract_table([((b"w",), SC), ((b"r",), I)], fetch=False)
        tcol = ctx.fetch_table_column(0, tnr, SC, tnb[0])
        first = check_marshal(ctx, w, kept[1], "under the products")
        # the selection, the string column, the list column and the table are as they were
        for a, b in zip(ctx.fetch_rows(nr, rows), selection):
            assert np.array_equal(a, b)
        same_column(S, ctx.fetch_path_strings(len(scol[2]), len(scol[1])), scol, "the string column after marshal_rows")
        for a, b in zip(ctx.fetch_path_list(len(lcol[2]), len(lcol[1]), I), lcol):
            assert np.array_equal(a, b)
        same_column(SC, ctx.fetch_table_column(0, tnr, SC, tnb[0]), tcol, "the table after marshal_rows")
        # MarshalJSON afterwards returns what it returns without the call, and takes the rows away; marshal_rows puts them back
        assert ctx.marshal_json() == whole
        raises_arg(lambda: ctx._check(L.sjhip_fetch_marshaled_rows(ctx._h, None, None)), "no rows")
        assert ctx.marshal_rows()[1] == first
        # the filter and the serializer evict the text
        out = np.empty(len(first) + 1, np.uint8)
        for evict in (lambda: ctx.filter_rows(fetch=False), lambda: ctx.serialize(fetch=False)):
            ctx.marshal_rows(fetch=False)
            evict()
            assert L.sjhip_fetch_marshaled(ctx._h, out.ctypes.data) == 5
            raises_arg(lambda: ctx._check(L.sjhip_fetch_marshaled_rows(ctx._h, None, out.ctypes.data)), "sjhip_marshal_rows")
    # a new parse drops the product, with the selection
    ctx.marshal_rows(fetch=False)
    ctx.parse(b'{"items":[[1],"s"]}', ndjson=True)
    raises_arg(lambda: ctx._check(L.sjhip_fetch_marshaled_rows(ctx._h, None, out.ctypes.data)), "sjhip_marshal_rows")
    raises_arg(ctx.marshal_rows, "no row selection")
    ctx.select_rows((b"items",))
    assert ctx.marshal_rows() == (2, b'[1]\n"s"')
    ctx.select_records()
    raises_arg(ctx.marshal_rows, "no row selection")
