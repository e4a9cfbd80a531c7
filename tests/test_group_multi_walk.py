"""CPU: the restated "group by" of several keys of tests/group_multi_walk.py (the checker of sjhip_group_paths), pinned with
hand-written expectations: column boundaries, swapped entries, every status on the second column with and without the null-key
flag, "no key" against the empty string, UINT and BOOL keys, several value columns, and -- with one column and no flag -- equality
with group_walk.group."""
import pytest

import column_walk as CW
import group_multi_walk as MW
import group_walk as GW
import rows_walk as RW
from test_group_walk import STATUS_DOC, rows_of
from test_rows_walk import walk_of

OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)
S, I, F, U, B = GW.COL_STRING, CW.COL_INT, CW.COL_FLOAT, CW.COL_UINT, CW.COL_BOOL
NONE = MW.GROUP_NONE


def test_column_boundaries_and_swapped_entries():
    rw = rows_of(b'{"rows":[{"a":"ab","b":"c"},{"a":"a","b":"bc"},{"a":"c","b":"ab"},{"a":"ab","b":"c"},{"a":"","b":"abc"}]}')
    g = MW.group(rw, [((b"a",), S), ((b"b",), S)])
    assert g.codes == [0, 1, 2, 0, 3] and g.first_row == [0, 1, 2, 4] and g.group_rows == [2, 1, 1, 1]
    assert g.keys == [[b"ab", b"a", b"c", b""], [b"c", b"bc", b"ab", b"abc"]] and g.key_ok == [[1] * 4, [1] * 4]
    assert MW.key_bytes(g, [S, S]) == [4, 8] and (g.rows, g.groups) == (5, 4)


# column "k" is group_walk's status document; column "j" is OK on every row that is an object
def test_every_status_on_the_second_column():
    rw = rows_of(STATUS_DOC.replace(b'{"', b'{"j":1,"'))
    plain = MW.group(rw, [((b"j",), I), ((b"k",), S)], [((b"v",), F), ((b"v",), I)])
    assert plain.status[0] == [OK, OK, NOT_OBJECT] + [OK] * 10
    assert plain.status[1] == [OK, NOT_FOUND, NOT_OBJECT, OK, NULL, TYPE, OK, TYPE, TYPE, OK, OK, TYPE, OK]
    assert plain.codes == [0, NONE, NONE, 1, NONE, NONE, 0, NONE, NONE, 2, 1, NONE, 0]
    assert plain.keys == [[1, 1, 1], [b"b", b"a", b""]] and plain.key_ok == [[1, 1, 1], [1, 1, 1]]
    assert [(a.count, a.not_ok, a.sum) for a in plain.aggs[0]] == [(1, 2, 1.0), (2, 0, 6.5), (1, 0, -3.0)]
    assert [(a.count, a.not_ok, a.sum) for a in plain.aggs[1]] == [(1, 2, 1), (2, 0, 6), (1, 0, -3)]
    flagged = MW.group(rw, [((b"j",), I), ((b"k",), S, True)])
    # NOT_FOUND, NULL, TYPE land in one group per key of column 0, numbered where it first occurs; row 2 is no object on column 0
    assert flagged.codes == [0, 1, NONE, 2, 1, 1, 0, 1, 1, 3, 2, 1, 0] and flagged.first_row == [0, 1, 3, 9]
    assert flagged.keys[1] == [b"b", None, b"a", b""] and flagged.key_ok[1] == [1, 0, 1, 1]  # "no key" is not the empty string
    assert MW.key_bytes(flagged, [I, S]) == [32, 2]
    both = MW.group(rw, [((b"j",), I, True), ((b"k",), S, True)])
    assert both.codes[2] == 2 and both.keys[0][2] is None and both.keys[1][2] is None and both.key_ok[0] == [1, 1, 0, 1, 1]
    assert both.groups == 5 and NONE not in both.codes


def test_uint_and_bool_keys_and_int_conversions():
    rw = rows_of(b'{"rows":[{"u":18446744073709551615,"b":true,"i":1},{"u":18446744073709551615,"b":false,"i":1.0},'
                 b'{"u":9223372036854775808,"b":true,"i":1.9},{"u":18446744073709551615,"b":true,"i":2},{"u":-1,"b":true,"i":1},'
                 b'{"u":1,"b":1,"i":1}]}')
    g = MW.group(rw, [((b"u",), U), ((b"b",), B), ((b"i",), I)])
    assert g.codes == [0, 1, 2, 3, NONE, NONE] and g.status[0][4] == RANGE and g.status[1][5] == TYPE and g.status[2] == [OK] * 6
    assert g.keys == [[(1 << 64) - 1, (1 << 64) - 1, 1 << 63, (1 << 64) - 1], [1, 0, 1, 1], [1, 1, 1, 2]]
    assert MW.key_bytes(g, [U, B, I]) == [32, 4, 32]
    one = MW.group(rw, [((b"i",), I)])
    assert one.keys == [[1, 2]] and one.codes == [0, 0, 0, 1, 0, 0]
    kinds = MW.group(rw, [((b"i",), S, True)])  # INT 1 is no STRING "1": every row is "no key"
    assert kinds.groups == 1 and kinds.key_ok == [[0]]


def test_empty_path_and_eight_columns():
    rw = rows_of(b'{"hashtags":["a","b","a",1,null,"b","a"]}', (b"hashtags",))
    g = MW.group(rw, [((), S), ((), S, True)])
    assert g.keys == [[b"a", b"b"], [b"a", b"b"]] and g.codes == [0, 1, 0, NONE, NONE, 1, 0]
    names = [b"c%d" % c for c in range(8)]
    row = lambda vals: "{" + ",".join('"c%d":%d' % (c, v) for c, v in enumerate(vals)) + "}"  # noqa: E731
    rows = [[0] * 8, [1] + [0] * 7, [0] * 4 + [1] + [0] * 3, [0] * 7 + [1], [0] * 8]
    rw = rows_of(('{"rows":[%s]}' % ",".join(map(row, rows))).encode())
    g = MW.group(rw, [((n,), I) for n in names])
    assert g.codes == [0, 1, 2, 3, 0] and [k[1:] for k in g.keys] == [[1, 0, 0]] + [[0] * 3] * 3 + [[0, 1, 0]] + [[0] * 3] * 2 + [[0, 0, 1]]
    with pytest.raises(ValueError):
        MW.group(rw, [((n,), I) for n in names] + [((b"c0",), I)])
    with pytest.raises(ValueError):
        MW.group(rw, [((b"c0",), F)])


@pytest.mark.parametrize("kind", [S, I])
def test_one_column_without_a_flag_is_group_walk(kind):
    for copy in (True, False):
        w = walk_of(STATUS_DOC, copy=copy)
        rw = RW.on_rows(w, (b"rows",))
        for vkind in (None, F, I, U):
            one = GW.group(rw, (b"k",), kind, (b"v",), vkind)
            g = MW.group(rw, [((b"k",), kind)], [] if vkind is None else [((b"v",), vkind)])
            assert (g.rows, g.groups, g.keys[0], g.status[0], g.first_row, g.group_rows, g.codes) == \
                (one.rows, one.groups, one.keys, one.status, one.first_row, one.group_rows, one.codes)
            assert g.key_ok == [[1] * one.groups]
            if vkind is not None:
                assert MW.arrays(g, 0, vkind) == GW.arrays(one, vkind)
