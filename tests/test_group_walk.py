"""CPU: the restated "group by" of tests/group_walk.py (the checker of sjhip_group_path), pinned with hand-written expectations: a
document whose rows hit every key status, "A" against its escaped spelling, the empty key, 1 / 1.0 / 1.9 as INT keys, a uint64 key
above int64 (RANGE: in no group), an empty path over scalar rows, and the aggregates per group."""
import aggregate_walk as AW
import column_walk as CW
import group_walk as GW
import rows_walk as RW
from test_rows_walk import walk_of

OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)
S, I, F, U = GW.COL_STRING, CW.COL_INT, CW.COL_FLOAT, CW.COL_UINT
NONE = GW.GROUP_NONE

# rows that hit every key status (STRING keys: no RANGE; INT keys: all six); tests/test_gpu_group.py runs the device on it
STATUS_ROWS = [
    '{"k":"b","v":1}',                       # 0
    '{"x":1}',                               # 1 the key is missing
    '7',                                     # 2 a row that is no object
    '{"k":"a","v":2.5}',                     # 3
    '{"k":null,"v":1}',                      # 4
    '{"k":12,"v":1}',                        # 5 STRING: TYPE; INT: the key 12
    '{"k":"b","v":"s"}',                     # 6 the value is not OK
    '{"k":18446744073709551615,"v":1}',      # 7 INT: RANGE
    '{"k":[1],"v":1}',                       # 8 TYPE
    '{"k":"","v":-3}',                       # 9 the empty key
    '{"k":"a","v":4}',                       # 10
    '{"k":12.9,"v":7}',                      # 11 INT: the key 12 again
    '{"k":"b"}',                             # 12 no value
]
STATUS_DOC = ('{"rows":[' + ",".join(STATUS_ROWS) + "]}").encode()


def rows_of(doc, path=(b"rows",)):
    w = walk_of(doc)
    return RW.on_rows(w, path)


def test_every_key_status():
    rw = rows_of(STATUS_DOC)
    g = GW.group(rw, (b"k",), S, (b"v",), F)
    assert g.status == [OK, NOT_FOUND, NOT_OBJECT, OK, NULL, TYPE, OK, TYPE, TYPE, OK, OK, TYPE, OK]
    assert g.keys == [b"b", b"a", b""] and g.first_row == [0, 3, 9] and g.group_rows == [3, 2, 1]
    assert g.codes == [0, NONE, NONE, 1, NONE, NONE, 0, NONE, NONE, 2, 1, NONE, 0] and (g.rows, g.groups) == (13, 3)
    assert [(a.count, a.not_ok, a.sum, a.min, a.max) for a in g.aggs] == [(1, 2, 1.0, 1.0, 1.0), (2, 0, 6.5, 2.5, 4.0), (1, 0, -3.0, -3.0, -3.0)]
    assert GW.arrays(g, F)[0] == [1, 2, 1] and GW.arrays(g, F)[1] == [2, 0, 0]
    i = GW.group(rw, (b"k",), I, (b"v",), I)
    assert i.status == [TYPE, NOT_FOUND, NOT_OBJECT, TYPE, NULL, OK, TYPE, RANGE, TYPE, TYPE, TYPE, OK, TYPE]
    assert i.keys == [12] and i.first_row == [5] and i.group_rows == [2] and i.codes.count(NONE) == 11
    assert (i.aggs[0].count, i.aggs[0].sum, i.aggs[0].min, i.aggs[0].max) == (2, 8, 1, 7)
    none = GW.group(rw, (b"nope",), S)  # no row has an OK key
    assert (none.rows, none.groups, none.keys, none.aggs) == (13, 0, [], None) and set(none.codes) == {NONE}


def test_escaped_and_empty_keys():
    for copy in (True, False):  # without copied strings "A" lies in the message and its escaped spelling in Strings.B
        w = walk_of(b'{"rows":[{"k":"A"},{"k":"\\u0041"},{"k":""},{"k":"a"},{"k":""},{"k":"\\u0041\\u0041"},{"k":"AA"}]}', copy=copy)
        g = GW.group(RW.on_rows(w, (b"rows",)), (b"k",), S)
        assert g.keys == [b"A", b"", b"a", b"AA"] and g.codes == [0, 0, 1, 2, 1, 3, 3]
        assert g.first_row == [0, 2, 3, 5] and g.group_rows == [2, 2, 1, 2]


def test_int_keys():
    rw = rows_of(b'{"rows":[{"k":1},{"k":1.0},{"k":1.9},{"k":-1},{"k":-1.5},{"k":9223372036854775808.0},'
                 b'{"k":18446744073709551615},{"k":-9223372036854775808},{"k":0},{"k":-0.0},{"k":"1"}]}')
    g = GW.group(rw, (b"k",), I)
    assert g.keys == [1, -1, -(1 << 63), 0]  # 2^63 as a float is the amd64 result MinInt64: the key of the true MinInt64 as well
    assert g.codes == [0, 0, 0, 1, 1, 2, NONE, 2, 3, 3, NONE] and g.status[6] == RANGE and g.status[10] == TYPE
    assert g.first_row == [0, 3, 5, 8] and g.group_rows == [3, 2, 2, 2]


def test_empty_path_over_scalar_rows():
    rw = rows_of(b'{"hashtags":["a","b","a",1,null,"b","a"],"n":[3,3.5,"3",4]}', (b"hashtags",))
    g = GW.group(rw, (), S)
    assert g.keys == [b"a", b"b"] and g.codes == [0, 1, 0, NONE, NONE, 1, 0] and g.status[3:5] == [TYPE, NULL]
    rw = rows_of(b'{"hashtags":["a","b","a",1,null,"b","a"],"n":[3,3.5,"3",4]}', (b"n",))
    g = GW.group(rw, (), I, (), U)  # key and value: the row's own value
    assert g.keys == [3, 4] and g.codes == [0, 0, NONE, 1] and [a.sum for a in g.aggs] == [6, 4]


def test_integer_sums_per_group_are_exact():
    hi = (1 << 63) - 1
    rw = rows_of(('{"rows":[%s]}' % ",".join('{"k":"%s","v":%d}' % ("xy"[r % 2], hi if r % 2 == 0 else -(1 << 63)) for r in range(6))).encode())
    g = GW.group(rw, (b"k",), S, (b"v",), I)
    assert [a.sum for a in g.aggs] == [3 * hi, -3 << 63]
    lo_hi = GW.arrays(g, I)
    assert (lo_hi[2][0], lo_hi[3][0]) == ((3 * hi) & AW.U64, 1) and lo_hi[3][1] == ((-3 << 63) >> 64) & AW.U64
    assert GW.GROUP_SORT_TILE == 1024 and GW.QTILE == 1024
