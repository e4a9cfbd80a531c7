"""GPU: row predicates over several tests (sjhip_where_paths, sjhip_count_where_paths) against the serial restatement of
tests/where_multi_walk.py over the oracle's parse: what fetch_rows delivers after the call and what the count says before it.  The
equivalences with sjhip_where_path bit for bit, every operator under OR, the seams of the wave (64), the block (256) and the scan
tile (1024), the limits of the plan and of the program, documents, no rows, the argument errors and a sharded result."""
import ctypes as C
import json
import struct

import numpy as np
import pytest

import fixtures
import query_walk as Q
import rows_walk as RW
import where_multi_walk as MW
import where_walk as WW
from test_gpu_columns import oracle_walk, random_nd
from test_gpu_parse import ctx  # noqa: F401
from test_gpu_rows import wrapped_random
from test_gpu_where import SEAM_COUNTS, WANT, seam_rows

pytestmark = pytest.mark.gpu

AND, OR, NEG = MW.WHERE_AND, MW.WHERE_OR, MW.WHERE_NEG
OK = 0


def check_multi(ctx, w, sel, predicates, program):
    """where_paths on the selection in force (sel: the walker's, None without one) equals the walker, and count_where_paths counted
    the rows it keeps without touching the selection; -> the walker's new selection"""
    program = bytes(program)
    want_off, want_idx, want_st = MW.where_multi(w, sel, predicates, program)
    assert ctx.count_where_paths(predicates, program) == len(want_idx), (predicates, program.hex())
    nr, rows = ctx.where_paths(predicates, program)
    assert (nr, rows) == (len(want_st), len(want_idx)), (predicates, program.hex(), nr, rows)
    off, idx, st = ctx.fetch_rows(nr, rows)
    assert off.dtype == np.uint64 and idx.dtype == np.uint64 and st.dtype == np.uint8
    assert st.tolist() == want_st and off.tolist() == want_off, (predicates, program.hex())
    assert np.array_equal(idx, np.array(want_idx, dtype=np.uint64)), (predicates, program.hex())
    return want_off, want_idx, want_st


def fetched(ctx, nr, rows):
    return [a.copy() for a in ctx.fetch_rows(nr, rows)]


def same_selection(a, b, what):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y), what


# ---- the equivalences with where_path, bit for bit, in both copy modes --------------------------------------------------------------
A_EXISTS = ((b"a",), Q.OP_EXISTS, None)
B_NULL = ((b"b",), Q.OP_IS_NULL, None)


def check_equivalences(ctx, w, base, reselect):
    for pred in (A_EXISTS, B_NULL, ((b"a", b"b"), WW.OP_GE_FLOAT, 0.0), ((b"",), WW.OP_PREFIX_STRING, b"")):
        path, op, want = pred
        for negate in (False, True):
            reselect()
            single = fetched(ctx, *ctx.where_path(path, op, want, negate=negate))
            reselect()
            sel = check_multi(ctx, w, base, [pred], [0, NEG] if negate else [0])
            same_selection(fetched(ctx, len(sel[2]), len(sel[1])), single, (pred, negate))
    reselect()
    ctx.where_path(*A_EXISTS)
    two = fetched(ctx, *ctx.where_path(*B_NULL, negate=True))  # two successive calls: the conjunction
    reselect()
    sel = check_multi(ctx, w, base, [A_EXISTS, B_NULL], [0, 1, NEG, AND])
    assert 0 < len(sel[1]) < 700
    same_selection(fetched(ctx, len(sel[2]), len(sel[1])), two, "a b NEG AND")
    ctx.where_path((b"a",), Q.OP_EQ_STRING, b"HOND")
    two = fetched(ctx, *ctx.where_path((b"a",), Q.OP_EQ_STRING, b"HOND"))
    reselect()
    ctx.where_path(*A_EXISTS)  # ... composed with an earlier call
    same_selection(fetched(ctx, *ctx.where_paths([B_NULL, ((b"a",), Q.OP_EQ_STRING, b"HOND")], bytes([0, NEG, 1, AND]))), two, "composition")
    ctx.select_records()


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_equivalences_on_items(ctx, copy):
    doc = wrapped_random(11, 700)
    w = oracle_walk(doc, True, copy)
    ctx.parse(doc, ndjson=True, copy_strings=copy)
    base = RW.select_rows(w, (b"items",))
    assert len(base[1]) == 700
    check_equivalences(ctx, w, base, lambda: ctx.select_rows((b"items",)))


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_equivalences_on_records(ctx, copy):
    doc = random_nd(11, 700)
    w = oracle_walk(doc, True, copy)
    ctx.parse(doc, ndjson=True, copy_strings=copy)
    check_equivalences(ctx, w, None, ctx.select_records)
    assert len(ctx.find_path(b"a")) == 700


# ---- every operator under OR ----------------------------------------------------------------------------------------------------------
OR_SEED, OR_ROWS = 1, 700  # (chosen once: on these records both sides of every OR below keep a row the other does not)


def test_every_operator_under_or(ctx):
    doc = random_nd(OR_SEED, OR_ROWS)
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    right = set(WW.where(w, None, *B_NULL)[1])
    for op in WW.ALL_OPS:
        pred = ((b"a",), op, WANT[op])
        left = set(WW.where(w, None, *pred)[1])
        assert left - right and right - left, op  # the OR is neither of its sides
        ctx.select_records()
        sel = check_multi(ctx, w, None, [pred, B_NULL], [0, 1, OR])
        assert set(sel[1]) == left | right, op
    ctx.select_records()


# ---- the seams of the wave, the block and the scan tile ---------------------------------------------------------------------------
def check_seams(ctx, w, base, reselect, n):
    """programs that keep every row, no row, only the last, every row but the first of a tile, every second, and the two rows at the
    scan tile's seam, each from two tests on the selection `base` (None: the records) put back in force by reselect()"""
    v, p, m = (b"v",), (b"p",), (b"m",)
    first_of_tile = 1024 if n > 1024 else 0
    for preds, program, kept in [
            ([(v, WW.OP_GE_INT, 0), (p, Q.OP_EQ_UINT, 7)], [0, 1, OR], n),
            ([(v, WW.OP_GE_INT, 0), (p, Q.OP_EQ_UINT, 7)], [0, 1, AND], 0),
            ([(v, WW.OP_GE_UINT, n - 1), (v, WW.OP_LT_INT, 0)], [0, 1, OR], 1),                         # only the last row
            ([(v, Q.OP_EQ_INT, first_of_tile), (p, Q.OP_EXISTS, None)], [0, NEG, 1, AND], n - 1),      # all but the first of a tile
            ([(p, Q.OP_EQ_UINT, 1), (v, WW.OP_GE_INT, 0)], [0, 1, AND], n // 2),
            ([(m, WW.OP_GT_FLOAT, 0.5), (v, Q.OP_EQ_INT, 1023), (v, Q.OP_EQ_INT, 1024)], [1, 2, OR, 0, AND], max(0, min(n, 1025) - 1023))]:
        reselect()
        sel = check_multi(ctx, w, base, preds, program)
        assert len(sel[1]) == kept, (n, preds, program)
    ctx.select_records()


@pytest.mark.parametrize("n", SEAM_COUNTS)
def test_record_counts_at_the_seams(ctx, n):
    doc = "\n".join(seam_rows(n)).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    check_seams(ctx, w, None, ctx.select_records, n)


@pytest.mark.parametrize("n", SEAM_COUNTS)
def test_row_counts_at_the_seams(ctx, n):
    doc = ("[" + ",".join(seam_rows(n)) + "]").encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    base = RW.select_rows(w, ())
    assert len(base[1]) == n
    check_seams(ctx, w, base, lambda: ctx.select_rows(()), n)


@pytest.mark.parametrize("n", (257, 1025, 2049))
def test_records_owning_0_to_7_rows(ctx, n):
    rows, lines, at, k = seam_rows(n), [], 0, 0
    while at < n:
        take = (k * 5) % 8
        lines.append('{"k":%d,"items":[%s]}' % (k, ",".join(rows[at:at + take])))
        at += take
        k += 1
    doc = "\n".join(lines).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    base = RW.select_rows(w, (b"items",))
    assert len(base[1]) == n and base[0] != list(range(len(base[0])))
    check_seams(ctx, w, base, lambda: ctx.select_rows((b"items",)), n)


# ---- the limits of the plan and of the program --------------------------------------------------------------------------------------
def nested(keys, leaf):
    text = leaf
    for k in reversed(keys):
        text = '{"%s":%s}' % (k, text)
    return text


def test_sixteen_predicates_and_the_deepest_program(ctx):
    lines = ["{" + ",".join('"k%d":%d' % (j, (r >> (j % 10)) & 1) for j in range(16) if (r + j) % 7) + "}" for r in range(300)]
    doc = "\n".join(lines).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    preds = [((b"k%d" % j,), Q.OP_EQ_INT, 1) for j in range(16)]
    for ops in ([OR] * 15, [AND, OR] * 7 + [OR], [OR, OR, AND] * 5):
        ctx.select_records()
        sel = check_multi(ctx, w, None, preds, list(range(16)) + ops)
        assert 0 < len(sel[1]) < 300
    # 32 pushes in front of 31 operators: the stack of the program is 32 deep
    for ops in ([OR, AND] * 15 + [OR], [AND] * 16 + [OR] * 15):
        ctx.select_records()
        program = [j % 16 for j in range(32)] + ops
        assert len(program) == 63
        sel = check_multi(ctx, w, None, preds, program)
        assert 0 < len(sel[1]) < 300
    ctx.select_records()


def test_the_deepest_path_and_the_widest_trie(ctx):
    deep = ["d%d" % j for j in range(16)]
    lines = []
    for r in range(130):
        cut = r % 18  # the path ends early at a number (a non-object on the way), is whole, or its last key is missing
        if cut < 15:
            lines.append(nested(deep[:cut + 1], "5"))
        elif cut == 15:
            lines.append(nested(deep, str(r)))
        elif cut == 16:
            lines.append(nested(deep[:15], '{"x":1}'))
        else:
            lines.append("[%d]" % r)
    doc = "\n".join(lines).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    path = tuple(k.encode() for k in deep)
    sel = check_multi(ctx, w, None, [(path, WW.OP_GE_INT, 50)], [0])  # 16 keys through 16 nested objects: the resume stack is full
    assert 0 < len(sel[1]) < 8
    ctx.select_records()
    sel = check_multi(ctx, w, None, [(path, WW.OP_GE_INT, 50)], [0, NEG])  # NOT_OBJECT and NOT_FOUND are false, and true under NEG
    assert len(sel[1]) > 120
    ctx.select_records()
    # paths that are the beginning of another (3 + 16 + 12 keys: the plan takes 32)
    preds = [(path[:3], Q.OP_EQ_INT, 5), (path, WW.OP_GE_INT, 30), (path[:12], Q.OP_EXISTS, None)]
    sel = check_multi(ctx, w, None, preds, [1, 0, OR, 2, NEG, AND])
    assert 0 < len(sel[1]) < 130
    ctx.select_records()
    # 32 trie nodes in all: two paths of 16 keys that share nothing
    other = tuple(b"e%d" % j for j in range(16))
    doc2 = "\n".join([nested(deep, "1"), nested(["e%d" % j for j in range(16)], '"s"'), '{"d0":{"d1":2},"e0":{"e1":{"e2":3}}}',
                      '{"d0":%s,"e0":%s}' % (nested(deep[1:], "1"), nested(["e%d" % j for j in range(1, 16)], '"s"'))]).encode()
    w2 = oracle_walk(doc2, True, True)
    ctx.parse(doc2, ndjson=True)
    preds = [(path, Q.OP_EQ_INT, 1), (other, Q.OP_EQ_STRING, b"s")]
    assert check_multi(ctx, w2, None, preds, [0, 1, OR])[0] == [0, 1, 2, 2, 3]
    ctx.select_records()
    assert check_multi(ctx, w2, None, preds, [0, 1, AND])[0] == [0, 0, 0, 0, 1]
    ctx.select_records()


def test_range_and_in_on_one_path(ctx):
    doc = fixtures.load("parking-citations")
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    makes = [b"HOND", b"TOYT", b"FORD", b"NISS"]
    sel = check_multi(ctx, w, None, [((b"Make",), Q.OP_EQ_STRING, m) for m in makes], [0, 1, OR, 2, OR, 3, OR])  # a 4-value IN
    recs = [json.loads(line) for line in doc.split(b"\n") if line.strip()]
    assert len(sel[1]) == sum(r.get("Make") in ("HOND", "TOYT", "FORD", "NISS") for r in recs) > 0
    ctx.select_records()
    doc = "\n".join('{"Fine":%s}' % v for v in ["49", "50", "50.5", "99", "100", "99.9", '"73"', "null", "1e2", "-60"] * 30).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    sel = check_multi(ctx, w, None, [((b"Fine",), WW.OP_GE_FLOAT, 50.0), ((b"Fine",), WW.OP_LT_FLOAT, 100.0)], [0, 1, AND])  # the range
    assert len(sel[1]) == 4 * 30
    ctx.select_records()


def test_empty_path_predicates(ctx):
    doc = b'{"prices":[1,2.5,"x",null]}\n{"prices":[]}\n{"prices":[-3,"xy",100,true]}'
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    base = RW.select_rows(w, (b"prices",))
    ctx.select_rows((b"prices",))
    preds = [((), WW.OP_GT_FLOAT, 2.0), ((), WW.OP_PREFIX_STRING, b"x"), ((), Q.OP_IS_NULL, None)]  # alone, on scalar rows
    sel = check_multi(ctx, w, base, preds, [0, 1, OR, 2, OR])
    assert sel[0] == [0, 3, 3, 5] and "".join(chr(w.t[i] >> 56) for i in sel[1]) == 'd"n"l'
    sel = check_multi(ctx, w, sel, [((), Q.OP_EQ_STRING, b"xy"), ((), Q.OP_EQ_INT, 100)], [0, 1, OR, NEG])  # a second call
    assert sel[0] == [0, 3, 3, 3]
    ctx.select_records()
    doc = wrapped_random(3, 300)  # mixed with path predicates, on object (and a few array) rows
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    base = RW.select_rows(w, (b"items",))
    ctx.select_rows((b"items",))
    sel = check_multi(ctx, w, base, [A_EXISTS, ((), Q.OP_EXISTS, None), ((), WW.OP_GE_INT, 0), B_NULL], [0, 1, AND, 2, NEG, AND, 3, NEG, AND])
    assert 0 < len(sel[1]) < 300
    ctx.select_records()


# ---- documents --------------------------------------------------------------------------------------------------------------------
def test_twitter_disjunction_then_a_narrowing(ctx):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    sel = RW.select_rows(w, (b"statuses",))
    ctx.select_rows((b"statuses",))
    sel = check_multi(ctx, w, sel, [((b"lang",), Q.OP_EQ_STRING, b"ja"), ((b"lang",), Q.OP_EQ_STRING, b"en")], [0, 1, OR])
    sel = check_multi(ctx, w, sel, [((b"retweet_count",), WW.OP_GE_INT, 1)], [0])
    want = [s for s in json.loads(doc)["statuses"] if s["lang"] in ("ja", "en") and s["retweet_count"] >= 1]
    assert 0 < len(want) == len(sel[1]) < 100
    assert ctx.extract_path((b"id",), ctx.COL_INT)[0].tolist() == [s["id"] for s in want]
    ctx.select_records()


def test_github_events_two_prefixes(ctx):
    doc = fixtures.load("github_events")
    w = oracle_walk(doc, False, True)
    events = json.loads(doc)
    ctx.parse(doc)
    sel = RW.select_rows(w, ())
    ctx.select_rows(())
    sel = check_multi(ctx, w, sel, [((b"type",), WW.OP_PREFIX_STRING, b"Push"), ((b"type",), WW.OP_PREFIX_STRING, b"Watch")], [0, 1, OR])
    want = [e for e in events if e["type"].startswith(("Push", "Watch"))]
    assert 0 < len(want) == len(sel[1]) < len(events)
    off, data, st = ctx.extract_path_strings((b"id",))
    assert [data[off[k]:off[k + 1]].decode() for k in range(len(want))] == [e["id"] for e in want]
    ctx.select_records()


# ---- no rows, errors, a sharded result ----------------------------------------------------------------------------------------------
def test_no_rows_kept_and_a_selection_without_rows(ctx):
    doc = random_nd(3, 200)
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    sel = check_multi(ctx, w, None, [((b"nope",), Q.OP_EXISTS, None), A_EXISTS], [0, 1, AND])
    assert sel == ([0] * 201, [], [OK] * 200)
    assert len(ctx.find_path(b"a")) == 0
    # on the selection without rows nothing is launched, and the sizes are right
    assert check_multi(ctx, w, sel, [A_EXISTS, B_NULL], [0, 1, OR]) == sel
    assert check_multi(ctx, w, sel, [A_EXISTS], [0, NEG]) == sel
    ctx.select_records()
    assert ctx.count_where_paths([A_EXISTS], bytes([0, NEG, 0, OR])) == 200


def test_argument_errors_touch_nothing(ctx):
    import sjhip
    doc = b'{"o":1,"items":[{"s":"abc","n":1},{"s":"de","n":2.5},{"s":"f","n":-3}]}\n{"o":2,"items":[{"n":null}]}'
    ctx.parse(doc, ndjson=True)
    ctx.select_rows((b"items",))
    assert ctx.where_paths([((b"n",), ctx.OP_LT_FLOAT, 2.0), ((b"s",), ctx.OP_EXISTS, None)], bytes([0, 1, AND])) == (2, 2)
    before = fetched(ctx, 2, 2)
    n_pred, s_pred = ((b"n",), ctx.OP_GE_INT, 1), ((b"s",), ctx.OP_EQ_STRING, b"abc")
    deep, many = ((b"k",) * 17, ctx.OP_EXISTS, None), [((b"k%d" % j, b"x", b"y"), ctx.OP_EXISTS, None) for j in range(11)]
    for preds, program, names in [
            ([], [0], "0 predicates"), ([n_pred] * 17, list(range(16)) + [OR] * 15, "17 predicates"),
            ([n_pred, ((b"s",), 20, None)], [0, 1, OR], "predicate 1"), ([((b"s",), -1, None), n_pred], [0, 1, OR], "predicate 0"),
            ([n_pred, deep], [0, 1, OR], "predicate 1"), (many, list(range(11)) + [OR] * 10, "predicate 10"),
            ([n_pred, ((b"s",), ctx.OP_EQ_STRING, b"x" * 1020)], [0, 1, OR], "predicate 1"),
            ([((b"k" * 600,), ctx.OP_EXISTS, None), ((b"j" * 600,), ctx.OP_EXISTS, None)], [0, 1, OR], "predicate 1"),
            ([n_pred, s_pred], [], "program"), ([n_pred], [0] + [NEG] * 64, "program"),
            ([n_pred, s_pred], [0, OR, 1], "position 1"), ([n_pred, s_pred], [AND, 0, 1], "position 0"),
            ([n_pred, s_pred], [0, 1], "position 2"), ([n_pred, s_pred], [0, 0, OR], "predicate 1"),
            ([n_pred, s_pred], [0, 2, OR], "position 1"), ([n_pred, s_pred], [0, 1, 0x83], "position 2")]:
        for call in (ctx.where_paths, ctx.count_where_paths):
            with pytest.raises(sjhip.ParseError) as e:
                call(preds, bytes(program))
            assert e.value.code == 5 and names in str(e.value), (names, str(e.value))
            same_selection(fetched(ctx, 2, 2), before, names)
    # a value of the wrong size: the mirror always packs the right one, so through the C call
    L, h = sjhip.lib(), ctx._h
    lens, plens, nr, nw = (C.c_uint32 * 2)(1, 1), (C.c_uint32 * 2)(1, 1), C.c_size_t(77), C.c_size_t(77)
    eight = struct.pack("<q", 1)
    for ops, vlens in [((ctx.OP_GE_INT, ctx.OP_EXISTS), (4, 0)), ((ctx.OP_EXISTS, ctx.OP_LE_FLOAT), (0, 0)), ((ctx.OP_EQ_BOOL, ctx.OP_EXISTS), (8, 0)),
                       ((ctx.OP_EXISTS, ctx.OP_IS_NULL), (0, 8)), ((ctx.OP_EXISTS, ctx.OP_EXISTS), (8, 0))]:
        bad = next(p for p in (0, 1) if vlens[p] != {ctx.OP_GE_INT: 8, ctx.OP_LE_FLOAT: 8, ctx.OP_EQ_BOOL: 1}.get(ops[p], 0))
        rc = L.sjhip_where_paths(h, b"ns", lens, plens, (C.c_int * 2)(*ops), eight, (C.c_uint32 * 2)(*vlens), 2, bytes([0, 1, OR]), 3,
                                 C.byref(nr), C.byref(nw))
        assert rc == 5 and ("predicate %d" % bad) in ctx.last_error(), (ops, vlens, ctx.last_error())
        same_selection(fetched(ctx, 2, 2), before, (ops, vlens))
    assert (nr.value, nw.value) == (77, 77)
    ctx.select_records()


@pytest.mark.parametrize("name", ["ABC", "BAB"])
def test_sharded_result_equals_whole(name):
    import test_gpu_product_parts as PP
    one, many = PP.contexts(name)
    I, SC = one.COL_INT, one.COL_STRING_CVT
    try:
        # (the stretches without values keep nothing under the first program: whole shards narrow to no rows)
        for preds, program in [([((b"s",), WW.OP_PREFIX_STRING, b"v5"), ((b"x",), WW.OP_GE_INT, 100)], [0, 1, AND]),
                               ([((b"x",), Q.OP_EXISTS, None), ((b"id",), WW.OP_LT_INT, 1000100)], [0, NEG, 1, OR])]:
            got = []
            for c in (one, many):
                c.select_records()
                count = c.count_where_paths(preds, bytes(program))
                nr, rows = c.where_paths(preds, bytes(program))
                assert count == rows
                sel = fetched(c, nr, rows)
                mid = int(np.median(c.extract_path((b"id",), I)[0]))
                nr2, rows2 = c.where_paths([((b"id",), WW.OP_GE_INT, mid), ((b"id",), WW.OP_LT_INT, 0)], bytes([0, 1, OR]))
                got.append((nr, rows, sel, nr2, rows2, fetched(c, nr2, rows2), c.extract_table([((b"id",), I), ((b"s",), SC)])))
            a, b = got
            assert a[:2] == b[:2] and a[3:5] == b[3:5] and 0 < a[4] < a[1] < a[0], (name, program, a[:2], a[3:5])
            PP.same(b[2], a[2], (name, program, "rows"))
            PP.same(b[5], a[5], (name, program, "rows, narrowed twice"))
            PP.same(b[6][0], a[6][0], (name, program, "id"))
            PP.same(b[6][1], a[6][1], (name, program, "s"))
    finally:
        one.select_records()
        many.select_records()
