"""CPU: the restated aggregates of tests/aggregate_walk.py (the checker of sjhip_aggregate_path / sjhip_aggregate_path_records),
pinned on fixtures -- twitter's statuses as rows with an INT and a UINT path, against Python's json as the outside arbiter;
parking-citations lines with a FLOAT path, whose members are all strings: every row is a type error and nothing is summed -- and on
a hand-written document whose rows hit every status.  The total is the reduction of column_walk.column and every record's entry the
reduction of its slice; min and max follow the key order, -0.0 below +0.0."""
import json
import math

import aggregate_walk as AW
import column_walk as CW
import fixtures
import rows_walk as RW
from test_rows_walk import walk_of

F, I, U = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT
OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)

# rows that hit every status; tests/test_gpu_aggregate.py runs the device on it
STATUS_ROWS = [
    '{"x":1}',                          # the key is missing
    '7',                                # a row that is no object
    '{"v":"12"}',                       # a string
    '{"v":null}', '{"v":true}', '{"v":[1,2]}',
    '{"v":-1}',                         # UINT: RANGE
    '{"v":9223372036854775808.0}',      # 2^63 as a float: INT gives MinInt64 and OK (the amd64 result)
    '{"v":1e300}',                      # INT and UINT: RANGE
    '{"v":18446744073709551616.0}',     # 2^64 as a float: UINT gives 0 and OK; INT: RANGE
    '{"v":18446744073709551615}',       # MaxUint64: INT RANGE
    '{"v":3}', '{"v":2.5}',
]
STATUS_DOC = ('{"rows":[' + ",".join(STATUS_ROWS) + "]}").encode()
STATUS_WANT = {  # kind: (status histogram, sum, min, max)
    F: ([7, 1, 1, 3, 1, 0], None, -1.0, 1e300),
    I: ([4, 1, 1, 3, 1, 3], -1 - (1 << 63) + 3 + 2, -(1 << 63), 3),
    U: ([5, 1, 1, 3, 1, 2], (1 << 63) + 0 + ((1 << 64) - 1) + 3 + 2, 0, (1 << 64) - 1),
}


def same(a, b):
    assert (a.rows, a.status, a.count, a.not_ok) == (b.rows, b.status, b.count, b.not_ok)
    assert (a.sum, a.min, a.max) == (b.sum, b.min, b.max)


def check_slices(rw, offs, path, kind):
    """total = the reduction of the column, per record = the reduction of its slice"""
    vals, sts = CW.column(rw, path, kind)
    same(AW.total(rw, path, kind), AW.reduce(vals, sts, kind))
    per = AW.per_record(rw, offs, path, kind)
    assert len(per) == len(offs) - 1
    for r, a in enumerate(per):
        same(a, AW.reduce(vals[offs[r]:offs[r + 1]], sts[offs[r]:offs[r + 1]], kind))
    assert sum(a.rows for a in per) == len(vals) and sum(a.count for a in per) == sts.count(OK)
    return per


def test_twitter_statuses():
    doc = fixtures.load("twitter")
    w = walk_of(doc)
    offs, index, sts = RW.select_rows(w, (b"statuses",))
    rw = RW.RowWalk(w, index)
    statuses = json.loads(doc)["statuses"]
    for path, kind, nums in [((b"retweet_count",), I, [s["retweet_count"] for s in statuses]),
                             ((b"user", b"followers_count"), U, [s["user"]["followers_count"] for s in statuses])]:
        per = check_slices(rw, offs, path, kind)
        a = AW.total(rw, path, kind)
        assert (a.rows, a.count, a.sum, a.min, a.max) == (len(nums), len(nums), sum(nums), min(nums), max(nums))
        assert len(per) == 1 and per[0].sum == sum(nums)
    # without a selection: one record, whose root holds no such member
    a = AW.per_record(w, None, (b"retweet_count",), I)
    assert len(a) == 1 and a[0].status[NOT_FOUND] == 1 and (a[0].count, a[0].sum, a[0].min) == (0, 0, None)


def test_parking_citations_float_path():
    doc = b"\n".join(fixtures.load("parking-citations").split(b"\n")[:200])
    w = walk_of(doc, nd=True)
    a = AW.total(w, (b"Fine",), F)  # "Fine":"50" is a string: Iter.Float refuses it
    assert a.rows == 200 and a.status[TYPE] == 200 and (a.count, a.sum, a.min, a.max) == (0, 0.0, None, None)
    per = check_slices(w, list(range(201)), (b"Fine",), F)
    assert AW.record_arrays(per, F) == ([0] * 200, [1] * 200) + ([0] * 200,) * 4
    assert AW.total(w, (b"Nope",), F).status[NOT_FOUND] == 200


def test_every_status():
    w = walk_of(STATUS_DOC)
    offs, index, sts = RW.select_rows(w, (b"rows",))
    rw = RW.RowWalk(w, index)
    assert offs == [0, len(STATUS_ROWS)]
    for kind, (hist, total, lo, hi) in STATUS_WANT.items():
        a = AW.total(rw, (b"v",), kind)
        assert a.status == hist and (a.min, a.max) == (lo, hi), (kind, a)
        if total is not None:
            assert a.sum == total, (kind, a)
        check_slices(rw, offs, (b"v",), kind)
    f = AW.total(rw, (b"v",), F)
    assert f.sum == math.fsum([-1.0, 2.0 ** 63, 1e300, 2.0 ** 64, 18446744073709551615.0, 3.0, 2.5])
    # segments cut inside: a record without rows, one without an OK row
    per = AW.per_record(rw, [0, 0, 2, 2, 7, len(STATUS_ROWS)], (b"v",), I)
    assert [(a.rows, a.count, a.sum, a.min, a.max) for a in per[:3]] == [(0, 0, 0, None, None), (2, 0, 0, None, None), (0, 0, 0, None, None)]
    assert AW.record_arrays(per[:2], I) == ([0, 0], [0, 2], [0, 0], [0, 0], [0, 0], [0, 0])
    assert (per[3].count, per[3].sum) == (1, -1) and per[4].sum == 5 - (1 << 63)


def test_empty_path_and_key_order():
    doc = b'{"k":{"v":[-0.0,0.0,-1.5,2.5,"s",null]},"o":[{"v":-0.0},{"v":0.0},{"v":-1.5},{"v":2.5},{"v":"s"},{"v":null}]}'
    w = walk_of(doc)
    bare = RW.on_rows(w, (b"k", b"v"))
    keyed = RW.on_rows(w, (b"o",))
    for kind in (F, I, U):
        a, b = AW.total(bare, (), kind), AW.total(keyed, (b"v",), kind)  # the row's own value: the same histogram as behind a key
        same(a, b)
        assert a.status[TYPE] == 1 and a.status[NULL] == 1
    a = AW.total(bare, (), F)
    assert (a.sum, a.min, a.max) == (1.0, -1.5, 2.5)
    zeros = RW.RowWalk(w, bare.rows[:2])
    z = AW.total(zeros, (), F)
    assert CW.f2bits(z.min) == 1 << 63 and CW.f2bits(z.max) == 0  # -0.0 ranks below +0.0
    assert AW.key(CW.f2bits(-0.0), F) < AW.key(CW.f2bits(0.0), F) < AW.key(CW.f2bits(5e-324), F)
    assert AW.key(CW.f2bits(-1.5), F) < AW.key(CW.f2bits(-5e-324), F) < AW.key(CW.f2bits(-0.0), F)
    assert AW.key((1 << 64) - 1, I) < AW.key(0, I) and AW.key(0, U) < AW.key((1 << 64) - 1, U)
    # 128 bits of an integer sum
    lo_hi = AW.record_arrays([AW.reduce([(1 << 64) - 1] * 3, [OK] * 3, U), AW.reduce([1 << 63] * 3, [OK] * 3, I)], U)
    assert (lo_hi[2][0], lo_hi[3][0]) == ((1 << 64) - 3, 2)
    assert (lo_hi[2][1], lo_hi[3][1]) == ((-3 << 63) & ((1 << 64) - 1), ((-3 << 63) >> 64) & ((1 << 64) - 1))
