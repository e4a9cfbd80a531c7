"""CPU: the restated "order by several keys" of tests/order_multi_walk.py (the checker of sjhip_order_paths), pinned with hand-written
tables -- a minor key that breaks the ties of the major one, mixed directions, the rows without a key last WITHIN their tie class, a
limit that only the second column or only the row order decides --, held against numpy.lexsort on numeric columns, and the serial
restatement of the device's plan (plan) held against the model on the families the GPU tests run.  The plan also says which rows
every column evaluated: what the device cannot show."""
import random

import numpy as np

import column_walk as CW
import order_multi_walk as MW
import order_strings_walk as SW
import order_walk as OW
import rows_walk as RW
from test_rows_walk import walk_of

OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)
F, I, U, S = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT, MW.COL_STRING


def rows_doc(rows):
    return ('{"rows":[%s]}' % ",".join(rows)).encode()


def ordered(rows, cols, limit=0):
    w = walk_of(rows_doc(rows))
    sel = RW.select_rows(w, (b"rows",))
    return MW.order(w, sel, cols, limit), sel, w


def test_the_second_key_breaks_the_ties_of_the_first():
    rows = ['{"m":"VW","f":30}', '{"m":"BMW","f":10}', '{"m":"VW","f":50}', '{"m":"BMW","f":70}', '{"m":"VW","f":30}', '{"m":"AUDI","f":5}']
    o, sel, _ = ordered(rows, [((b"m",), S, False), ((b"f",), I, True)])
    assert o.order == [5, 3, 1, 2, 0, 4] and o.status == [OK] * 6 and o.values is None and o.selection == sel
    o, _, _ = ordered(rows, [((b"m",), S, True), ((b"f",), I, False)])
    assert o.order == [0, 4, 2, 1, 3, 5]  # the two (VW, 30) in row order
    o, _, _ = ordered(rows, [((b"f",), F, False), ((b"m",), S, False)])
    assert o.order == [5, 1, 0, 4, 2, 3]


def test_rows_without_a_key_are_last_within_their_class():
    rows = ['{"a":1,"b":"x"}', '{"a":1}', '{"b":"a"}', '{"a":1,"b":"c"}', '{"a":0,"b":null}', '{"a":0,"b":"z"}', '{"b":7}', '7', '{"a":"s","b":"a"}']
    o, _, _ = ordered(rows, [((b"a",), I, False), ((b"b",), S, False)])
    # a = 0: z, then null; a = 1: c, x, then the row without b; no a: "a" (rows 2 and 8 tie on both: row order), then 6 and 7
    assert o.order == [5, 4, 3, 0, 1, 2, 8, 6, 7]
    assert o.status == [OK] * 5 + [NOT_FOUND, TYPE, NOT_FOUND, NOT_OBJECT]  # column 0's
    o, _, _ = ordered(rows, [((b"a",), I, True), ((b"b",), S, True)])
    assert o.order == [0, 3, 1, 5, 4, 2, 8, 6, 7]


def test_a_limit_that_only_a_later_column_or_the_row_order_decides():
    rows = ['{"a":1,"b":3}', '{"a":1,"b":1}', '{"a":1,"b":2}', '{"a":0,"b":9}', '{"a":1,"b":1}']
    o, sel, _ = ordered(rows, [((b"a",), U, False), ((b"b",), U, False)], limit=2)
    assert o.order == [1, 0] and o.selection[1] == [sel[1][1], sel[1][3]]  # (0, 9), then the first (1, 1)
    o, _, _ = ordered(rows, [((b"a",), U, False), ((b"b",), U, False)], limit=4)
    assert o.order == [2, 0, 3, 1] and o.rows == 4  # row 0 (1, 3) is cut


def test_one_column_is_the_single_key_checkers():
    rows = ['{"k":"b","v":2}', '{"k":"a","v":-1.5}', '{"v":2}', '{"k":"b","v":null}', '{"k":"","v":2.0}']
    w = walk_of(rows_doc(rows))
    sel = RW.select_rows(w, (b"rows",))
    for desc in (False, True):
        for limit in (0, 3):
            a, b = MW.order(w, sel, [((b"k",), S, desc)], limit), SW.order(w, sel, (b"k",), desc, limit)
            assert (a.order, a.status, a.selection) == (b.order, b.status, b.selection)
            a, b = MW.order(w, sel, [((b"v",), F, desc)], limit), OW.order(w, sel, (b"v",), F, desc, limit)
            assert (a.order, a.status, a.selection) == (b.order, b.status, b.selection)


def numeric_data(rnd, n, spec):
    """spec: [(kind, descending, distinct values)] -> the checker's column data, every status OK"""
    data = []
    for kind, desc, distinct in spec:
        vals = [rnd.randrange(distinct) - distinct // 2 if kind == I else rnd.randrange(distinct) for _ in range(n)]
        data.append((kind, desc, [v & MW.U64 for v in vals], [OK] * n))
    return data


def test_agrees_with_lexsort():
    rnd = random.Random(5)
    for n, spec in ((1, [(I, False, 3)] * 2), (200, [(I, False, 5), (U, True, 4), (I, True, 1000)]), (500, [(U, True, 3), (I, False, 3), (U, False, 3)])):
        data = numeric_data(rnd, n, spec)
        signed = [np.array(keys, dtype=np.uint64).astype(np.int64) if kind == I else np.array(keys, dtype=np.uint64).astype(np.float64)
                  for kind, _, keys, _ in data]
        lex = np.lexsort([-(a.astype(np.float64)) if desc else a.astype(np.float64) for a, (_, desc, _, _) in list(zip(signed, data))[::-1]])
        assert MW.rank(data, n) == lex.tolist()
        assert MW.plan(data, n)[0] == lex.tolist()


def pattern_data(n, pattern):
    first = {"all-equal": lambda r: 7, "all-distinct": lambda r: (r * 7919) % 100003, "pairs": lambda r: (r + 1) // 2,
             "three-classes": lambda r: 1 if r == n // 2 else (0 if r % 2 else 2)}[pattern]
    return [(I, False, [first(r) for r in range(n)], [OK] * n), (U, True, [(r * 31) % 17 for r in range(n)], [OK] * n)]


def test_the_plan_gives_the_rank_and_walks_only_the_ties():
    for n in (1, 2, 63, 64, 65, 300):
        for pattern in ("all-equal", "all-distinct", "pairs", "three-classes"):
            data = pattern_data(n, pattern)
            perm, evaluated, rounds = MW.plan(data, n)
            assert perm == MW.rank(data, n), (n, pattern)
            assert evaluated[0] == list(range(n))
            if pattern == "all-distinct" or n == 1:
                assert len(evaluated) == 1  # column 1 evaluates no row
            elif pattern == "all-equal":
                assert evaluated[1] == list(range(n))
            elif pattern == "pairs":  # rows 2 j - 1 and 2 j share a key; row 0, and the last row of an even count, are alone
                assert evaluated[1:] == [p for p in [[r for r in range(1, n) if r % 2 == 1 and r + 1 < n or r % 2 == 0]] if p], (n, evaluated[1:])
            elif n > 2:
                assert n // 2 not in evaluated[1] and len(evaluated[1]) == n - 1


def test_the_plan_on_strings_statuses_and_eight_columns():
    rnd = random.Random(9)
    stem = "abcdefghijklmnopqrstu"
    for trial in range(6):
        n = 240
        lengths = (0, 6, 7, 8, 13, 14, 15, 21)
        names = [(stem[:max(length - 1, 0)] + rnd.choice("ux"))[:length] for length in lengths for _ in range(3)] + [stem[:length] for length in lengths]
        s_keys = [rnd.choice(names).encode() for _ in range(n)]
        s_sts = [rnd.choice((OK, OK, OK, OK, NOT_FOUND, NULL, TYPE)) for _ in range(n)]
        i_sts = [rnd.choice((OK, OK, OK, RANGE, NOT_OBJECT)) for _ in range(n)]
        data = [(S, trial % 2 == 1, [k if st == OK else None for k, st in zip(s_keys, s_sts)], s_sts),
                (I, trial % 3 == 1, [rnd.randrange(4) if st == OK else 0 for st in i_sts], i_sts),
                (S, trial % 2 == 0, [rnd.choice((b"", b"a", b"abcdefg", b"abcdefgh")) for _ in range(n)], [OK] * n)]
        for order in (data, data[1:] + data[:1], data[::-1]):
            perm, evaluated, rounds = MW.plan(order, n)
            assert perm == MW.rank(order, n), trial
            assert all(set(b) <= set(a) for a, b in zip(evaluated, evaluated[1:]))  # a later column sees a subset
    # the different-rounds family alone: the ties of column 0 end in rounds 1 .. 4 and meet again in column 1
    keys = [stem[:length].encode() for length in (0, 6, 7, 8, 13, 14, 15, 21) for _ in range(3)]
    rnd.shuffle(keys)
    data = [(S, False, keys, [OK] * 24), (I, True, list(range(24)), [OK] * 24)]
    perm, evaluated, rounds = MW.plan(data, 24)
    assert perm == MW.rank(data, 24) and rounds == [4, 1] and evaluated[1] == list(range(24))
    # eight columns, the first seven tie in shrinking classes: column c splits every class of column c - 1 in two
    n = 256
    data = [(U, c % 2 == 1, [(r >> (7 - c)) & 1 for r in range(n)], [OK] * n) for c in range(7)] + [(U, True, [r % 2 for r in range(n)], [OK] * n)]
    perm, evaluated, rounds = MW.plan(data, n)
    assert perm == MW.rank(data, n) and [len(e) for e in evaluated] == [n] * 8 and rounds == [1] * 8
    # every row without a key everywhere: row order, one round per column (the class ties as a whole)
    data = [(I, False, [0] * 5, [NOT_FOUND] * 5), (S, True, [None] * 5, [TYPE] * 5)]
    assert MW.plan(data, 5) == ([0, 1, 2, 3, 4], [[0, 1, 2, 3, 4]] * 2, [1, 1])


def test_class_key_and_stays():
    assert MW.class_key(1, False) == 2 and MW.class_key(1, True) == 3 and MW.class_key(1 << 30, True) == (1 << 31) + 1
    assert MW.stays(False, False, True) and not MW.stays(True, False, True) and not MW.stays(False, True, True) and not MW.stays(False, False, False)
    assert MW.ORDER_MAX_KEYS == 8 and MW.COL_STRING == 4 and MW.ORDER_DESC == 1
