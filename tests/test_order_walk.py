"""CPU: the restated "order by ... limit k" of tests/order_walk.py (the checker of sjhip_order_path), pinned with hand-written
expectations -- ties, the pair -0.0 / +0.0, the stability of a descending order, the rows without an OK key last in both directions,
a limit that cuts a run of ties, the narrowing under a selection of several records -- and against numpy's stable argsort on random
keys."""
import random

import numpy as np

import column_walk as CW
import order_walk as OW
import rows_walk as RW
from test_group_walk import STATUS_DOC
from test_rows_walk import walk_of

OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)
F, I, U = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT


def ordered(doc, path, kind, descending=False, limit=0, rows=(b"rows",), key=(b"k",)):
    w = walk_of(doc)
    sel = RW.select_rows(w, rows)
    return OW.order(w, sel, key, kind, descending, limit), sel


def rows_doc(values):
    return ('{"rows":[%s]}' % ",".join('{"k":%s}' % v for v in values)).encode()


def test_ties_stay_in_row_order_in_both_directions():
    doc = rows_doc([3, 1, 3, 2, 1, 3])
    o, sel = ordered(doc, None, I)
    assert o.order == [1, 4, 3, 0, 2, 5] and o.values == [1, 1, 2, 3, 3, 3] and o.status == [OK] * 6 and (o.records, o.rows) == (1, 6)
    assert o.selection == sel  # no limit: the selection is as it was
    o, _ = ordered(doc, None, I, descending=True)
    assert o.order == [0, 2, 5, 3, 1, 4] and o.values == [3, 3, 3, 2, 1, 1]  # not the ascending list reversed


def test_zeros_and_mixed_numbers_under_float():
    doc = rows_doc(["0.0", "-0.0", "0", "-1e308", "5e-324", "-5e-324", "1", "1.0"])
    o, _ = ordered(doc, None, F)
    assert o.order == [3, 5, 1, 0, 2, 4, 6, 7]  # -0.0 below +0.0; 0.0 and the integer 0 tie, 1 and 1.0 tie: row order
    assert o.values[2] == 1 << 63 and o.values[3] == 0 and o.values[4] == 0
    o, _ = ordered(doc, None, F, descending=True)
    assert o.order == [6, 7, 4, 0, 2, 1, 5, 3]
    o, _ = ordered(doc, None, I)  # truncated to equal int64 keys: 0, 0, 0, RANGE, 0, 0, 1, 1
    assert o.order == [0, 1, 2, 4, 5, 6, 7, 3] and o.status[-1] == RANGE and o.values[-1] == 0


def test_rows_without_an_ok_key_are_last_in_both_directions():
    w = walk_of(STATUS_DOC)
    sel = RW.select_rows(w, (b"rows",))
    # "v": 1, -, (no object), 2.5, 1, 1, "s", 1, 1, -3, 4, 7, -
    o = OW.order(w, sel, (b"v",), F)
    assert o.order == [9, 0, 4, 5, 7, 8, 3, 10, 11, 1, 2, 6, 12]
    assert o.status == [OK] * 9 + [NOT_FOUND, NOT_OBJECT, TYPE, NOT_FOUND]
    assert [CW.bits2f(b) for b in o.values] == [-3.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.5, 4.0, 7.0, 0.0, 0.0, 0.0, 0.0]
    o = OW.order(w, sel, (b"v",), F, descending=True)
    assert o.order == [11, 10, 3, 0, 4, 5, 7, 8, 9, 1, 2, 6, 12]
    o = OW.order(w, sel, (b"k",), I)  # the key 12 twice, RANGE, and every other status
    assert o.order[:2] == [5, 11] and o.order[2:] == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 12]
    assert sorted(set(o.status)) == [OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE]


def test_limit_cuts_a_run_of_ties_and_narrows_in_document_order():
    doc = rows_doc([5, 1, 5, 5, 0, 5])
    o, sel = ordered(doc, None, U, limit=3)
    # ranks: rows 4, 1, 0, 2, 3, 5 -- the first of the four 5s crosses the limit
    assert o.rows == 3 and o.selection[0] == [0, 3] and o.selection[1] == [sel[1][0], sel[1][1], sel[1][4]]
    assert o.order == [2, 1, 0] and o.values == [0, 1, 5]
    o, _ = ordered(doc, None, U, descending=True, limit=3)
    assert o.selection[1] == [sel[1][0], sel[1][2], sel[1][3]] and o.order == [0, 1, 2] and o.values == [5, 5, 5]
    for limit in (6, 7, 0):
        o, _ = ordered(doc, None, U, limit=limit)
        assert o.rows == 6 and o.selection == sel
    # a limit beyond the OK rows keeps rows without a key, in row order
    o, _ = ordered(rows_doc(['"x"', 2, "null", 1]), None, I, limit=3)
    assert o.order == [2, 1, 0] and o.status == [OK, OK, TYPE] and o.selection[0] == [0, 3]


def test_records_keep_the_rows_they_owned():
    doc = b'{"items":[4,9,1]}\n{"items":[]}\n{"x":1}\n{"items":[7]}\n{"items":[8,2]}'
    w = walk_of(doc, nd=True)
    sel = RW.select_rows(w, (b"items",))
    assert sel[0] == [0, 3, 3, 3, 4, 6] and sel[2] == [OK, OK, NOT_FOUND, OK, OK]
    o = OW.order(w, sel, (), I, descending=True, limit=3)  # 9, 8, 7
    assert o.selection[0] == [0, 1, 1, 1, 2, 3] and o.selection[2] == sel[2] and o.records == 5
    assert o.selection[1] == [sel[1][1], sel[1][3], sel[1][4]] and o.order == [0, 2, 1] and o.values == [9, 8, 7]
    # without a selection the records are the rows and a selection is created
    o = OW.order(w, None, (b"x",), I, limit=2)
    assert o.selection[0] == [0, 1, 1, 2, 2, 2] and o.selection[2] == [OK] * 5 and o.order == [1, 0] and o.status == [OK, NOT_FOUND]


def test_against_a_stable_argsort():
    rnd = random.Random(5)
    for kind, dtype, gen in [(I, np.int64, lambda: rnd.randrange(-(1 << 63), 1 << 63) if rnd.random() < 0.5 else rnd.randrange(-3, 3)),
                             (U, np.uint64, lambda: rnd.randrange(0, 1 << 64) if rnd.random() < 0.5 else rnd.randrange(0, 4)),
                             (F, np.float64, lambda: rnd.choice((-1.0, 1.0)) * 10.0 ** rnd.uniform(-300, 300) if rnd.random() < 0.5 else float(rnd.randrange(-2, 3)))]:
        xs = [gen() for _ in range(500)]
        o, _ = ordered(rows_doc([repr(x) for x in xs]), None, kind)
        a = np.array(xs, dtype=dtype)
        assert o.order == np.argsort(a, kind="stable").tolist()
        assert np.array(o.values, dtype=np.uint64).view(dtype).tolist() == np.sort(a, kind="stable").tolist()
        o, _ = ordered(rows_doc([repr(x) for x in xs]), None, kind, descending=True)
        # descending and stable: the ascending stable order of the reversed list, read backwards
        want = (len(xs) - 1 - np.argsort(a[::-1], kind="stable"))[::-1]
        assert o.order == want.tolist()


def test_pass_mask_and_constants():
    ok = [OK] * 3
    assert OW.pass_mask([1, 2, 3], ok, U) == 1 and OW.pass_mask([7, 7, 7], ok, U) == 0 and OW.pass_mask([5], [OK], U) == 0
    assert OW.pass_mask([0, 1 << 20, 5], ok, U) == 0b101 and OW.pass_mask([0, 1 << 20, 5], ok, U, True) == 0b101
    assert OW.pass_mask([1, (-1) & OW.U64, 0], ok, I) == 0xFF and OW.pass_mask([1, 9, 1 << 40], [OK, TYPE, NULL], U) == 0
    assert OW.ORDER_SORT_TILE == 1024 and OW.QTILE == 1024 and OW.ORDER_DESC == 1
