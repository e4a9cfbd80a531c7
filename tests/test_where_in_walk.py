"""CPU: the restated set predicate of tests/where_in_walk.py (the checker of sjhip_where_path_in).  The definition -- a row is kept
iff any(EQ(row, s) for s in set), one single-predicate test (where_walk.satisfies) per value -- is pinned by json.loads navigation
on twitter statuses (user.screen_name, user.id, lang) and parking lines (Make); the one-conversion shortcut the GPU tests run
(key_of(row) in set) is pinned against the definition on a hand-written document of every edge; and every constructed family of
where_in_walk.families() really contains what it names: a collision, a wrapped chain, a probe that ends at the empty slot behind a
whole chain, a row that differs from a set value only in its last byte."""
import json

import column_walk as CW
import fixtures
import group_table as GT
import rows_walk as RW
import where_in_walk as IW
from test_rows_walk import walk_of

S, I, U = IW.COL_STRING, CW.COL_INT, CW.COL_UINT
OK = 0

EDGE_DOC = b"\n".join([
    b'{"x":1}',                              # 0  the key is missing
    b'{"a":5}',                              # 1  a non-object on the way
    b'[1]',                                  # 2  ... and at the root
    b'{"a":{"v":null}}',                     # 3
    b'{"a":{"v":"1"}}',                      # 4  a string where a number is asked for
    b'{"a":{"v":1}}',                        # 5
    b'{"a":{"v":1.0}}',                      # 6
    b'{"a":{"v":1.9}}',                      # 7  Int and Uint truncate: 1
    b'{"a":{"v":-1}}',                       # 8  a range error under UINT
    b'{"a":{"v":9223372036854775808}}',      # 9  2^63: a range error under INT
    b'{"a":{"v":18446744073709551615}}',     # 10 2^64 - 1: a range error under INT
    b'{"a":{"v":9223372036854775808.0}}',    # 11 the float 2^63: MinInt64 under INT (the amd64 result)
    b'{"a":{"v":{"k":1}}}',                  # 12 an object
    b'{"a":{"v":"A"}}',                      # 13
    b'{"a":{"v":"\\u0041"}}',                # 14 A, escaped
    b'{"a":{"v":""}}',                       # 15
    b'{"a":{"v":-1.5}}',                     # 16 -1 under INT
])
PATH = (b"a", b"v")
EDGE_SETS = [  # (kind, values, the records kept)
    (I, [1], [5, 6, 7]), (U, [1], [5, 6, 7]), (I, [-1], [8, 16]), (U, [(1 << 64) - 1], [10]), (I, [(1 << 64) - 1], [8, 16]),  # (the bits of -1)
    (U, [1 << 63], [9, 11]), (I, [1 << 63], [11]), (I, [-(1 << 63)], [11]), (U, [1 << 63, (1 << 64) - 1, 1], [5, 6, 7, 9, 10, 11]),
    (S, [b"1"], [4]), (S, [b"A"], [13, 14]), (S, [b""], [15]), (S, [b"A", b"", b"A", b"zz"], [13, 14, 15]), (S, [b"\\u0041"], []),
    (I, [], []), (S, [], []), (I, [1, 1, 1, -1, 1], [5, 6, 7, 8, 16]),
]


def test_edges_by_hand_and_the_shortcut_is_the_definition():
    w = walk_of(EDGE_DOC, nd=True)
    roots = w.records()
    n = len(roots)
    assert n == 17
    for kind, values, kept in EDGE_SETS:
        for negate in (False, True):
            expect = [r for r in range(n) if (r in kept) != negate]
            for by_definition in (True, False):
                offs, index, sts = IW.where_in(w, None, PATH, kind, values, negate, by_definition)
                assert index == [roots[r] + 1 for r in expect], (kind, values, negate, by_definition)
                assert sts == [OK] * n and offs == [sum(e < r for e in expect) for r in range(n + 1)], (kind, values, negate)


def test_narrowing_a_selection_and_scalar_rows():
    doc = b'{"tags":["a","b","a",1,null]}\n{"tags":[]}\n{"tags":["c","b"]}'
    w = walk_of(doc, nd=True)
    sel = RW.select_rows(w, (b"tags",))
    assert sel[0] == [0, 5, 5, 7]
    got = IW.where_in(w, sel, (), S, [b"a", b"c"])
    assert got[0] == [0, 2, 2, 3] and got[1] == [sel[1][0], sel[1][2], sel[1][5]] and got[2] == sel[2]
    rest = IW.where_in(w, sel, (), S, [b"a", b"c"], negate=True)
    assert rest[0] == [0, 3, 3, 4] and sorted(got[1] + rest[1]) == sel[1]
    assert IW.where_in(w, got, (), S, [b"c"])[0] == [0, 0, 0, 1]  # a second call narrows further


def test_twitter_statuses_against_json_navigation():
    doc = fixtures.load("twitter")
    w = walk_of(doc, nd=False)
    statuses = json.loads(doc)["statuses"]
    sel = RW.select_rows(w, (b"statuses",))
    assert len(sel[1]) == len(statuses)
    names = [s["user"]["screen_name"] for s in statuses]
    ids = [s["user"]["id"] for s in statuses]
    for path, kind, values, want in [
            ((b"user", b"screen_name"), S, [n.encode() for n in names[::3]] + [b"nobody"], [n in set(names[::3]) for n in names]),
            ((b"user", b"id"), I, ids[::5] + [7], [i in set(ids[::5]) for i in ids]),
            ((b"user", b"id"), U, ids[1::4], [i in set(ids[1::4]) for i in ids]),
            ((b"lang",), S, [b"ja", b"en", b"ja"], [s["lang"] in ("ja", "en") for s in statuses])]:
        assert 0 < sum(want) < len(want)
        for by_definition in (True, False):
            got = IW.where_in(w, sel, path, kind, values, False, by_definition)
            assert got[1] == [v for v, keep in zip(sel[1], want) if keep], (path, kind, by_definition)
            assert got[0] == [0, sum(want)] and got[2] == sel[2]


def test_parking_lines_against_json_navigation():
    doc = fixtures.load("parking-citations")
    lines = [line for line in doc.split(b"\n") if line.strip()][:400]
    w = walk_of(b"\n".join(lines), nd=True)
    makes = [json.loads(line).get("Make") for line in lines]
    values = [b"HOND", b"TOYT", b"BMW", b"HOND"]
    want = [m in ("HOND", "TOYT", "BMW") for m in makes]
    assert 0 < sum(want) < len(want)
    roots = w.records()
    for by_definition in (True, False):
        for negate in (False, True):
            got = IW.where_in(w, None, (b"Make",), S, values, negate, by_definition)
            assert got[1] == [r + 1 for r, keep in zip(roots, want) if keep != negate]


def test_set_values_are_read_as_the_kind_reads_them():
    assert IW.set_values(I, [(1 << 64) - 1, 1 << 63, 5]) == [-1, -(1 << 63), 5]
    assert IW.set_values(U, [-1, 1 << 63]) == [(1 << 64) - 1, 1 << 63]
    assert IW.EQ_OF == {4: 1, 1: 2, 2: 3} and IW.WHERE_IN_MAX_VALUES == 1 << 24 and IW.MAX_STRING == 1024


def test_every_family_contains_what_it_names():
    fams = IW.families()
    assert {"home63_int", "home63_str", "home120_int", "home120_str", "collide16", "collide19", "collide24", "twins"} == set(fams)
    for name, f in fams.items():
        values = IW.set_values(f.kind, f.values)
        assert GT.capacity(len(values)) == f.capacity, name
        kept = f.kept()
        assert any(kept) and not all(kept), name
        # the table, filled in index order and in reverse: the occupied slots do not depend on the order
        for order in (None, list(range(len(values)))[::-1]):
            filled = GT.model(values, f.capacity - 1, order)
            if f.chain is not None:
                assert set(filled.table) == f.chain, (name, sorted(filled.table))
            assert filled.wrapped == f.wraps, name
            probes = [IW.probe(f.kind, values, k, filled) for k in f.keys if k is not None]
            assert [p.found for p in probes] == [k for k, key in zip(kept, f.keys) if key is not None], name
            misses = [p for p in probes if not p.found]
            assert max(p.steps for p in misses) >= f.long_miss and sum(p.false_hits for p in misses) >= f.false_hits, (name, misses)
            if f.wraps:
                assert any(p.wrapped for p in probes if p.found) and any(p.wrapped for p in misses), name
    assert fams["home63_int"].capacity == 64 and fams["home120_int"].capacity == 128 and len(fams["home120_str"].values) == 33
    # a stranger homed in the middle of a chain ends at the empty slot behind it
    f = fams["home63_int"]
    mid = [IW.probe(f.kind, f.values, k) for k in f.keys[-5:-1]]
    assert all(not p.found and p.steps == 22 for p in mid), mid
    # collisions: one 64-bit hash, other bytes; with an equal first word; with a tail
    for name, length in (("collide16", 16), ("collide19", 19), ("collide24", 24)):
        f = fams[name]
        assert len({GT.hash_bytes(k) for k in f.keys + f.values}) == 1 and len(set(f.keys)) == 4 and all(len(k) == length for k in f.keys)
    assert len({k[:8] for k in fams["collide24"].keys}) == 1 and fams["collide19"].keys[0][16:] == fams["collide19"].keys[1][16:]
    # twins: the last byte only, the length only
    f = fams["twins"]
    n = len(f.values)
    for b, twin, shorter, longer in zip(f.keys[:n], f.keys[n:2 * n], f.keys[2 * n:3 * n], f.keys[3 * n:]):
        assert twin[:-1] == b[:-1] and twin[-1] != b[-1] and shorter == b[:-1] and longer[:-1] == b
    assert f.kept() == [True] * n + [False] * (3 * n)
