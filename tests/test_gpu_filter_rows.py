"""GPU: sjhip_filter_rows -- the selected rows as a self-contained (Tape, Strings.B) -- against the serial restatement of
tests/filter_rows_walk.py over the oracle's parse, and against the oracle's ParseND of the rows' texts where those are known:
parity under select_rows and where_path, equivalence with sjhip_filter_where, the fixtures, the seams of the row count (the
wave-per-row blocks of 4, the wave, the block, the 1024-row scan tile) and of the row length (the 64-word groups, the
short / long threshold), raw words that look like tags, one long row, the edge cases of Strings.B, scalar rows, errors and
the lifecycle."""
import json

import numpy as np
import pytest

import filter_rows_walk as FW
import fixtures
import query_walk as Q
import rows_walk as RW
import where_walk as WW
from test_filter_rows_walk import SCALAR_ROWS, items_doc, kinds_rows, oracle_of
from test_gpu_columns import oracle_walk, random_nd
from test_gpu_parse import ctx  # noqa: F401
from test_gpu_rows import RAW
from test_gpu_tables import KINDS6, same_column

pytestmark = pytest.mark.gpu

F, I, U, B, S, SC = KINDS6
FROWS_SHORT = 128  # csrc/query.hip: the words of a row its lane measures alone; a longer row is measured by its wave


def check_filter(ctx, w, rows, texts=None, what=None):
    """filter_rows on the selection in force -- whose row index is `rows` -- equals the restatement, and the oracle's parse of
    `texts` (the texts of the container rows) where they are known; -> the device's ParsedJson"""
    tape, strings, skipped = FW.filter_rows(w, rows)
    boxes = sum(chr(w.t[int(v)] >> 56) in "{[" for v in rows)
    n, sk, sizes = ctx.filter_rows(fetch=False)
    assert (n, sk, sizes) == (boxes, skipped, (len(tape), len(strings))), (what, n, sk, sizes)
    n, sk, pj = ctx.filter_rows()
    assert (n, sk) == (boxes, skipped), what
    assert pj.Tape.dtype == np.uint64 and pj.Strings.dtype == np.uint8
    assert np.array_equal(pj.Tape, np.array(tape, dtype=np.uint64)), what
    assert np.array_equal(pj.Strings, np.frombuffer(strings, dtype=np.uint8)), what
    if texts is not None:
        want = oracle_of(texts)
        assert np.array_equal(pj.Tape, want[0]) and np.array_equal(pj.Strings, want[1]), what
    return pj


def texts_at(w, rows, all_rows, order):
    """the texts of the container rows among `rows`, given the texts `order` of `all_rows`"""
    text = dict(zip(all_rows, order))
    return [text[v] for v in rows if chr(w.t[v] >> 56) in "{["]


# ---- parity -----------------------------------------------------------------------------------------------------------------------
def test_parity_on_items(ctx):
    doc, order, box = items_doc(kinds_rows(150), scalars_every=9)
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    sel = RW.select_rows(w, (b"items",))
    all_rows = sel[1]
    assert ctx.select_rows((b"items",))[1] == len(all_rows) == len(order)
    check_filter(ctx, w, all_rows, texts_at(w, all_rows, all_rows, order), "every row")
    for negate in (False, True):
        ctx.select_rows((b"items",))
        kept = WW.where(w, sel, (b"r",), WW.OP_GE_INT, 40, negate)
        assert ctx.where_path((b"r",), ctx.OP_GE_INT, 40, negate=negate)[1] == len(kept[1]) > 0
        check_filter(ctx, w, kept[1], texts_at(w, kept[1], all_rows, order), ("r >= 40", negate))
    ctx.select_rows((b"items",))
    kept = WW.where(w, sel, (b"r",), WW.OP_GE_INT, 40, False)
    kept = WW.where(w, kept, (b"w",), WW.OP_PREFIX_STRING, b"row 1", False)  # two successive calls: the conjunction
    ctx.where_path((b"r",), ctx.OP_GE_INT, 40)
    assert ctx.where_path((b"w",), ctx.OP_PREFIX_STRING, b"row 1")[1] == len(kept[1]) > 0
    check_filter(ctx, w, kept[1], texts_at(w, kept[1], all_rows, order), "r >= 40 and w has the prefix")
    ctx.select_records()


# ---- equivalence with the existing filter -----------------------------------------------------------------------------------------
def check_equals_filter_where(ctx, doc, key, value, matches=None):
    ctx.parse(doc, ndjson=True)
    n, sub = ctx.filter_where(key, value)
    assert matches is None or n == matches
    ctx.where_path((key,), ctx.OP_EQ_STRING, value)
    n2, skipped, pj = ctx.filter_rows()
    assert (n2, skipped) == (n, 0) and n > 0
    assert np.array_equal(pj.Tape, sub.Tape) and np.array_equal(pj.Strings, sub.Strings)
    ctx.select_records()


def test_equals_filter_where_on_parking(ctx):
    check_equals_filter_where(ctx, fixtures.load("parking-citations") * 3, b"Make", b"HOND", 348)  # (116 in one copy of the fixture)


def test_equals_filter_where_on_random_records(ctx):
    check_equals_filter_where(ctx, random_nd(11, 1500), b"a", b"HOND")


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def test_twitter_statuses(ctx):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = RW.select_rows(w, (b"statuses",))
    ctx.select_rows((b"statuses",))
    check_filter(ctx, w, sel[1], None, "statuses")
    kept = WW.where(w, sel, (b"retweet_count",), WW.OP_GE_INT, 10, False)
    assert ctx.where_path((b"retweet_count",), ctx.OP_GE_INT, 10)[1] == len(kept[1])
    want = [s for s in json.loads(doc)["statuses"] if s["retweet_count"] >= 10]
    assert 0 < len(want) == len(kept[1]) < 100
    pj = check_filter(ctx, w, kept[1], None, "retweet_count >= 10")
    sub = Q.Walk(pj.Tape, pj.Strings, b"")  # the result read as a ParsedJson: one root per status
    roots = sub.records()
    assert [sub.string_at(sub.find_path(r, [b"user", b"screen_name"])).decode() for r in roots] == [s["user"]["screen_name"] for s in want]
    ctx.select_records()


def test_canada_rings(ctx):
    """the coordinate rings of canada.json -- arrays of arrays of numbers, no string at all -- as the rows"""
    doc = fixtures.load("canada")
    start = doc.index(b'"coordinates":') + len(b'"coordinates":')
    end = doc.rindex(b"]", 0, doc.rindex(b"]"))
    doc = b'{"coordinates":' + doc[start:end + 1] + b"}"
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rows = RW.select_rows(w, (b"coordinates",))[1]
    assert ctx.select_rows((b"coordinates",))[1] == len(rows) > 100
    pj = check_filter(ctx, w, rows, None, "rings")
    assert len(pj.Strings) == 0 and len(pj.Tape) == len(w.t) - 8 + 2 * len(rows)  # (r { "coordinates" [ ... ] } r around them)
    ctx.select_records()


# ---- the seams of the row count ---------------------------------------------------------------------------------------------------
ROW_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_at_the_seams(ctx, n):
    texts = ['{"v":%d,"s":"%s"}' % (r, "t" * (r % 7) + str(r)) if r % 5 else '[%d,{"a":1}]' % r for r in range(n)]
    doc = ("[" + ",".join(texts) + "]").encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rows = RW.select_rows(w, ())[1]
    assert ctx.select_rows(()) == (1, n) and len(rows) == n
    pj = check_filter(ctx, w, rows, texts, n)
    assert len(pj.Tape) == len(w.t) - 4 + 2 * n
    ctx.select_records()


# ---- the seams of the row length, and raw words that look like tags -------------------------------------------------------------
RAWS = list(RAW.values()) + [(ord("r") << 56) + 12345]  # integers whose value word has the top byte [ { ] } l " r
ROW_LENGTHS = sorted(set(list(range(62, 67)) + list(range(126, 131)) + [FROWS_SHORT - 1, FROWS_SHORT, FROWS_SHORT + 1] +
                         list(range(190, 195)) + list(range(254, 259))))


def sized_row(words, ones, strings, seed=0):
    """an array row of exactly `words` tape words: [ , `ones` one-word atoms, two-word entries, ] -- the two-word entries are
    integers whose value words look like tags; strings: "none", "first" (the first two-word entry is a string: the last group of a
    long row holds none), "last" (the row's final entry is one), "both".  With ones even the two-word entries start at an odd
    index, so one of them straddles every 64-word group; with ones odd they are aligned to the groups."""
    twos = words - 2 - ones
    assert twos >= 4 and twos % 2 == 0
    items = [str(RAWS[(seed + k) % len(RAWS)]) for k in range(twos // 2)]
    if strings in ("first", "both"):
        items[0] = '"first of %d"' % words
    if strings in ("last", "both"):
        items[-1] = '"last of %d"' % words
    return "[" + ",".join(["true", "null", "false"][:ones] + items) + "]"


def sized_rows():
    texts, lengths = [], []
    for k, words in enumerate(ROW_LENGTHS):
        for ones in ((0, 2) if words % 2 == 0 else (1, 3)):
            for strings in ("none", "first", "last", "both"):
                row = sized_row(words, ones, strings, k)
                if (k + ones) % 4 == 3:  # ... and some as the value of an object's member: four words more
                    row = sized_row(words - 4, ones, strings, k)
                    row = '{"k%d":%s}' % (words, row)
                texts.append(row)
                lengths.append(words)
    return texts, lengths


def check_row_lengths(ctx):
    texts, lengths = sized_rows()
    doc = ("[" + ",".join(texts) + "]").encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rows = RW.select_rows(w, ())[1]
    assert [(w.t[v] & Q.MASK) - v for v in rows] == lengths  # every row is as long as it was meant to be
    assert ctx.select_rows(())[1] == len(rows)
    check_filter(ctx, w, rows, texts, "row lengths")
    # ... and with the object rows of every third of their lengths dropped: gaps in the tape and in Strings.B in front of the rows behind them
    sel = RW.select_rows(w, ())
    keys = sorted({t[2:t.index('"', 2)] for t in texts if t[0] == "{"})
    assert len(keys) > 6
    for key in [k.encode() for k in keys[::3]]:
        sel = WW.where(w, sel, (key,), Q.OP_EXISTS, None, True)
        ctx.where_path((key,), ctx.OP_EXISTS, negate=True)
    assert 0 < len(sel[1]) < len(rows)
    check_filter(ctx, w, sel[1], texts_at(w, sel[1], rows, texts), "row lengths, narrowed")
    ctx.select_records()


def test_row_lengths_at_the_seams(ctx):
    check_row_lengths(ctx)


def check_raw_words(ctx):
    """numbers whose value word looks like a tag, directly in the rows and nested, in rows of every length around the groups: copied
    as they are, never rebased (the restatement walks entry by entry and never looks at a raw word)"""
    vals = RAWS
    texts = []
    for k in range(200):
        v = vals[k % len(vals)]
        texts.append('{"a":%d,"b":[%d,{"a":%d}],"c":{"a":%d},"s":"x%d"}' % (v, vals[(k + 1) % 7], vals[(k + 2) % 7], v, k) if k % 2
                     else "[%s]" % ",".join(str(vals[(k + j) % 7]) for j in range(28 + k % 9)))  # 58 .. 74 words
    doc = ("\n".join('{"items":[%s]}' % ",".join(texts[k:k + 5]) for k in range(0, 200, 5))).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    rows = RW.select_rows(w, (b"items",))[1]
    assert ctx.select_rows((b"items",))[1] == 200 == len(rows)
    check_filter(ctx, w, rows, texts, "raw words")
    ctx.select_records()


def test_raw_words_that_look_like_tags(ctx):
    check_raw_words(ctx)


def test_one_long_row_between_short_ones(ctx):
    big = "[" + ",".join('"s%d"' % k if k % 1000 == 7 else str(RAWS[k % 7]) for k in range(50001)) + "]"
    texts = ["[]", "{}", big, "[]", '{"a":"after"}']
    doc = ("[" + ",".join(texts) + "]").encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rows = RW.select_rows(w, ())[1]
    assert (w.t[rows[2]] & Q.MASK) - rows[2] >= 100000
    ctx.select_rows(())
    check_filter(ctx, w, rows, texts, "one long row")
    ctx.select_records()


# ---- Strings.B ---------------------------------------------------------------------------------------------------------------------
def test_strings_edge_cases(ctx):
    """rows whose only strings are empty (keys included), rows without strings between rows with strings, kept rows behind dropped
    rows that own strings: the gaps in Strings.B close up"""
    texts = ['{"":""}', '["",""]', "[1,2]", '{"k":"owns bytes"}', "[[],{}]", '{"":["",{"":""}]}', '{"d":"dropped, with strings"}', "[3]",
             '{"q":"kept behind a gap"}', '{"d":["dropped again"]}', '{"":""}', '["the last"]']
    doc = ("[" + ",".join(texts) + "]").encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    all_rows = RW.select_rows(w, ())[1]
    for steps, kept_texts in [([], texts),
                              ([((b"d",), True)], [t for t in texts if '"d"' not in t]),
                              ([((b"",), False)], [texts[0], texts[5], texts[10]]),
                              ([((b"",), True), ((b"d",), True)], [texts[k] for k in (1, 2, 3, 4, 7, 8, 11)]),
                              ([((b"q",), False)], [texts[8]])]:
        sel = RW.select_rows(w, ())
        ctx.select_rows(())
        for path, negate in steps:
            sel = WW.where(w, sel, path, Q.OP_EXISTS, None, negate)
            ctx.where_path(path, ctx.OP_EXISTS, negate=negate)
        assert texts_at(w, sel[1], all_rows, texts) == kept_texts, steps
        check_filter(ctx, w, sel[1], kept_texts, steps)
    ctx.select_records()


# ---- scalars ------------------------------------------------------------------------------------------------------------------------
def test_scalar_rows(ctx):
    texts = ['{"a":1}', '"s"', "7", "[]", "null", '["x"]', "true", "2.5", '{"b":"y"}', '""']
    doc = ("[" + ",".join(texts) + "]").encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    rows = RW.select_rows(w, ())[1]
    ctx.select_rows(())
    n, skipped, pj = ctx.filter_rows()
    assert (n, skipped) == (4, 6)
    check_filter(ctx, w, rows, [t for t in texts if t[0] in "{["], "scalars and containers")  # the order is kept
    doc = ("[" + ",".join(SCALAR_ROWS) + "]").encode()  # scalars only: an empty result
    ctx.parse(doc)
    ctx.select_rows(())
    n, skipped, pj = ctx.filter_rows()
    assert (n, skipped, len(pj.Tape), len(pj.Strings)) == (0, len(SCALAR_ROWS), 0, 0)
    assert ctx.filter_rows(fetch=False) == (0, len(SCALAR_ROWS), (0, 0))
    doc = b"[" + b",".join([b"[]"] * 300) + b"]"  # two-word rows become four-word records: larger than the source tape
    w = oracle_walk(doc, False, True)
    tape_len = len(ctx.parse(doc).Tape)
    ctx.select_rows(())
    pj = check_filter(ctx, w, RW.select_rows(w, ())[1], ["[]"] * 300, "larger than the source")
    assert len(pj.Tape) == 1200 > tape_len == 604
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
    raises_arg(fresh.filter_rows)  # no result at all
    doc = b'{"k":"v","items":[{"a":"x"},{"a":"y"}]}\n{"k":"w","items":[{"a":"z"}]}'
    # no selection; the refused call touches no product: the filtered result of sjhip_filter_where is still there
    fresh.parse(doc, ndjson=True)
    n, sub = fresh.filter_where(b"k", b"v")
    assert n == 1
    raises_arg(fresh.filter_rows, "no row selection")
    tape, strings = np.empty(len(sub.Tape), np.uint64), np.empty(len(sub.Strings), np.uint8)
    assert L.sjhip_fetch_filtered(fresh._h, tape.ctypes.data, strings.ctypes.data) == 0
    assert np.array_equal(tape, sub.Tape) and np.array_equal(strings, sub.Strings)
    # a parse without copied strings; the selection and a column built before the call are as they were
    fresh.parse(doc, ndjson=True, copy_strings=False)
    fresh.select_rows((b"items",))
    before = fresh.fetch_rows(2, 3)
    col = fresh.extract_path_strings((b"a",))
    raises_arg(fresh.filter_rows, "SJHIP_FLAG_COPY_STRINGS")
    for a, b in zip(fresh.fetch_rows(2, 3), before):
        assert np.array_equal(a, b)
    same_column(S, fresh.fetch_path_strings(3, 3), col, "the column after a refused filter_rows")
    fresh.close()
    # a sharded result
    line = b'{"items":[{"a":"' + b"x" * 200 + b'"}]}'
    big = b"\n".join([line] * (3 * (1 << 20) // len(line)))
    with fixtures.nd_shard_limits(2 << 20, 1 << 20):
        many = sjhip.Context(0)
        many.parse(big, ndjson=True)
    rows = many.select_rows((b"items",))[1]
    assert rows > 1000
    raises_arg(many.filter_rows, "sjhip_filter_rows", "shard by shard")
    assert len(many.find_path(b"a")) == rows  # (the selection is still in force)
    many.close()


def test_lifecycle(ctx):
    import sjhip
    doc, order, box = items_doc(kinds_rows(90), scalars_every=11)
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True, key_flags=True)
    sel = RW.select_rows(w, (b"items",))
    nr, rows = ctx.select_rows((b"items",))
    kept = WW.where(w, sel, (b"r",), WW.OP_GE_INT, 30, False)
    nr, rows = ctx.where_path((b"r",), ctx.OP_GE_INT, 30)
    selection = ctx.fetch_rows(nr, rows)
    scol = ctx.extract_path_strings((b"w",), cvt=True)
    lcol = ctx.extract_path_list((b"v",), I)
    tnr, tnb = ctx.extract_table([((b"w",), SC), ((b"r",), I)], fetch=False)
    tcol = ctx.fetch_table_column(0, tnr, SC, tnb[0])
    first = check_filter(ctx, w, kept[1], None, "under the products")
    # the selection, the string column, the list column and the table are as they were
    for a, b in zip(ctx.fetch_rows(nr, rows), selection):
        assert np.array_equal(a, b)
    same_column(S, ctx.fetch_path_strings(len(scol[2]), len(scol[1])), scol, "the string column after filter_rows")
    for a, b in zip(ctx.fetch_path_list(len(lcol[2]), len(lcol[1]), I), lcol):
        assert np.array_equal(a, b)
    same_column(SC, ctx.fetch_table_column(0, tnr, SC, tnb[0]), tcol, "the table after filter_rows")
    # repeated calls give the same bytes; any out-pointer may be null
    again = ctx.filter_rows()[2]
    assert np.array_equal(again.Tape, first.Tape) and np.array_equal(again.Strings, first.Strings)
    L = sjhip.lib()
    assert L.sjhip_filter_rows(ctx._h, None, None, None, None) == 0
    tape, strings = np.empty(len(first.Tape), np.uint64), np.empty(max(len(first.Strings), 1), np.uint8)
    assert L.sjhip_fetch_filtered(ctx._h, tape.ctypes.data, strings.ctypes.data) == 0
    assert np.array_equal(tape, first.Tape) and np.array_equal(strings[:len(first.Strings)], first.Strings)
    # it replaces the result of sjhip_filter_where and is replaced by it
    n, sub = ctx.filter_where(b"pre", b"x")
    assert n == 0
    assert ctx.filter_rows(fetch=False)[2] == (len(first.Tape), len(first.Strings))
    # the serializer and MarshalJSON evict it
    for evict in (lambda: ctx.serialize(fetch=False), lambda: ctx.marshal_json(fetch=False)):
        ctx.filter_rows(fetch=False)
        evict()
        raises_arg(lambda: ctx._check(L.sjhip_fetch_filtered(ctx._h, tape.ctypes.data, strings.ctypes.data)), "no filtered result")
    # a new parse drops it, with the selection
    ctx.filter_rows(fetch=False)
    ctx.parse(b'{"items":[[1]]}', ndjson=True)
    raises_arg(lambda: ctx._check(L.sjhip_fetch_filtered(ctx._h, tape.ctypes.data, strings.ctypes.data)), "no filtered result")
    raises_arg(ctx.filter_rows, "no row selection")
    ctx.select_rows((b"items",))
    n, skipped, pj = ctx.filter_rows()
    assert (n, skipped) == (1, 0) and np.array_equal(pj.Tape, oracle_of(["[1]"])[0])
    ctx.select_records()
    raises_arg(ctx.filter_rows, "no row selection")
