"""CPU: the plan and the one-walk evaluation of a table (sjhip_extract_table).  tests/table_walk.py -- the restatement -- is pinned
per column against column_walk.column / string_column (FindElement + the conversions, one path at a time); the C++ the kernel
runs (csrc/sj_table.h, csrc/sj_tablewalk.h through sj_selftest_table_plan / sj_selftest_table_walk of host_selftest.cpp) is
checked against the restatement: the same nodes in the same order, the same tape index or path status for every column of every
record, in both copy modes of the oracle's parse; and every limit is refused beyond it and accepted at it."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as G
import column_walk as CW
import oracle_lib as O
import query_walk as Q
import table_walk as TW
from test_gpu_columns import RANDOM_PATHS, random_nd

F, I, U, B, S, SC = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT, CW.COL_BOOL, TW.COL_STRING, TW.COL_STRING_CVT
KINDS6 = (F, I, U, B, S, SC)

# ---- the hand-written documents ------------------------------------------------------------------------------------------------
EDGE_DOC = b"\n".join([
    b'{"a":{"b":1,"c":"x"},"s":"t","a":5}',              # a path that is the beginning of another; a second "a" that must not count
    b'{"a":1,"a":{"b":2}}',                               # the first "a" is no object: a.b is NOT_OBJECT, whatever follows
    b'{"a":{"c":1},"a":{"b":3}}',                         # the first "a" is an object without "b": a.b is NOT_FOUND
    b'[1,2]',                                             # a root array
    b'{}',                                                # an empty root object
    b'{"":7,"\\u0061":{"b":"esc"},"a":{"b":"plain"}}',    # the empty key; "a" is "a", and comes first
    b'{"a":{"b":{"c":null}},"b":true}',
    b'{"b":false,"s":"","a":{"b":18446744073709551616.0,"b":1}}',
    b'{"s":null,"a":[{"b":1}]}',                          # not into arrays
    b'{"a":{"b":{"c":true},"c":"y"}}',
])
EDGE_COLUMNS = [((b"a",), I), ((b"a", b"b"), I), ((b"a", b"b"), SC), ((b"a",), SC), ((b"s",), S), ((b"",), U),
                ((b"a", b"b", b"c"), B), ((b"b",), B), ((b"a", b"c"), S), ((b"a", b"b"), U)]

WIDE_KEYS = [b"k%d" % j for j in range(16)]
WIDE_DOC = b"\n".join([
    b'{' + b",".join(b'"k%d":%d' % (j, j * 3) for j in range(16)) + b'}',
    b'{' + b",".join(b'"k%d":"%d"' % (j, j) for j in reversed(range(16))) + b'}',
    b'{"k3":true,"k15":null,"k0":1.5,"k3":2}',
])
WIDE_COLUMNS = [((k,), KINDS6[j % 6]) for j, k in enumerate(WIDE_KEYS)]  # 16 columns

DEEP_PATH = tuple(b"p%d" % j for j in range(16))


def nested(path, leaf, around=b""):
    doc = leaf
    for key in reversed(path):
        doc = b'{' + around + b'"' + key + b'":' + doc + b'}'
    return doc


DEEP_DOC = b"\n".join([
    nested(DEEP_PATH, b"42"),
    nested(DEEP_PATH[:8], b'{"p8":"level 9 is a string"}', around=b'"z":0,'),  # everything below level 9 is NOT_OBJECT
    nested(DEEP_PATH, b'"leaf"', around=b'"z":[1],'),
    nested(DEEP_PATH[:5], b'{}'),
])
# 16 columns, a 16-key path, exactly 32 keys in all
DEEP_COLUMNS = ([(DEEP_PATH, I), (DEEP_PATH[:2], SC)] + [(DEEP_PATH[:1], k) for k in KINDS6] + [((b"z",), k) for k in KINDS6] +
                [((b"",), I), ((b"",), S)])
# ... and its prefixes, again exactly 32 keys
PREFIX_COLUMNS = [(DEEP_PATH[:d], k) for d, k in ((10, SC), (1, SC), (9, S), (4, I), (8, SC))]

RANDOM_COLUMNS = [(p, KINDS6[j % 6]) for j, p in enumerate(RANDOM_PATHS)]  # one 9-column table

CASES = [("edges", EDGE_DOC, EDGE_COLUMNS), ("wide", WIDE_DOC, WIDE_COLUMNS), ("deep", DEEP_DOC, DEEP_COLUMNS),
         ("prefixes", DEEP_DOC, PREFIX_COLUMNS), ("same path twice", EDGE_DOC, [((b"a", b"b"), I), ((b"a", b"b"), SC)]),
         ("one column", EDGE_DOC, [((b"s",), S)])]


def test_the_cases_are_at_the_limits():
    assert len(WIDE_COLUMNS) == 16 and len(DEEP_COLUMNS) == 16 and len(DEEP_PATH) == 16
    for cols in (DEEP_COLUMNS, PREFIX_COLUMNS):
        assert sum(len(p) for p, _ in cols) == 32


def parsed(doc, copy):
    ref = O.parse(doc, ndjson=True, copy_strings=copy)
    assert ref.rc == 0
    msg = doc[ref.msg_off:ref.msg_off + ref.msg_len]
    return Q.Walk(ref.tape, ref.strings, msg), ref, msg


_random = {}


def random_parsed(copy):
    if copy not in _random:
        _random[copy] = parsed(random_nd(11, 3000), copy)
    return _random[copy]


# ---- the restatement against the single columns ----------------------------------------------------------------------------------
def check_against_single_columns(w, columns):
    got = TW.table(w, columns)
    for (path, kind), col in zip(columns, got):
        assert col == TW.single(w, path, kind), (path, kind)


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_restatement_equals_the_single_columns(copy):
    for name, doc, columns in CASES:
        w, _, _ = parsed(doc, copy)
        check_against_single_columns(w, columns)
    w, _, _ = random_parsed(copy)
    check_against_single_columns(w, RANDOM_COLUMNS)


def test_hand_written_answers():
    w, _, _ = parsed(EDGE_DOC, True)
    NF, NO = Q.NOT_FOUND, Q.NOT_OBJECT
    rows = TW.indexes(w, [((b"a", b"b"), I), ((b"a",), I), ((b"a", b"b", b"c"), B)])
    kinds = [[v if v >= NO else "hit" for v in row] for row in rows]
    assert kinds == [["hit", "hit", NO], [NO, "hit", NO], [NF, "hit", NF], [NO, NO, NO], [NF, NF, NF], ["hit", "hit", NO],
                     ["hit", "hit", "hit"], ["hit", "hit", NO], [NO, "hit", NO], ["hit", "hit", "hit"]]
    (vals, sts), = TW.table(w, [((b"a", b"b"), I)])
    assert vals[:3] == [1, 0, 0] and sts[:3] == [CW.COL_OK, CW.COL_NOT_OBJECT, CW.COL_NOT_FOUND]
    (offs, data, sts), = TW.table(w, [((b"a", b"b"), SC)])
    assert data[:4] == b"1esc" and offs[:8] == [0, 1, 1, 1, 1, 1, 4, 4] and sts[5] == CW.COL_OK and sts[6] == CW.COL_TYPE


def test_every_status_occurs_in_the_random_table():
    """what tests/test_gpu_columns.py asserts for this seed and these paths over the oracle's parse, on the CPU"""
    w, _, _ = random_parsed(True)
    seen = set()
    for path in RANDOM_PATHS:
        for kind in (F, I, U, B):
            seen |= set(CW.column(w, path, kind)[1])
    assert seen == set(range(6)), seen
    seen = set()
    for col in TW.table(w, RANDOM_COLUMNS):
        seen |= set(col[-1])
    assert seen == set(range(6)), seen


# ---- the C++ the kernel runs ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cxx():
    lib = C.CDLL(G.build_selftest())
    lib.sj_selftest_table_plan.restype = C.c_int
    lib.sj_selftest_table_plan.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]
    lib.sj_selftest_table_walk.restype = C.c_int
    lib.sj_selftest_table_walk.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    return lib


def c_columns(columns):
    keys = [bytes(k) for path, _ in columns for k in path]
    return (b"".join(keys), np.array([len(k) for k in keys] + [0], dtype=np.uint32),
            np.array([len(p) for p, _ in columns] + [0], dtype=np.uint32), np.array([k for _, k in columns] + [0], dtype=np.int32))


def cxx_plan(lib, columns):
    """-> (nodes, root_n) shaped like table_walk.plan's, or the code the table was refused with"""
    blob, key_lens, path_lens, kinds = c_columns(columns)
    nodes = np.zeros((32, 6), dtype=np.uint32)
    out_blob = np.zeros(1024, dtype=np.uint8)
    n, root_n = C.c_uint32(0), C.c_uint32(0)
    rc = lib.sj_selftest_table_plan(blob, key_lens.ctypes.data, path_lens.ctypes.data, kinds.ctypes.data, len(columns), C.byref(n),
                                    C.byref(root_n), nodes.ctypes.data, out_blob.ctypes.data)
    if rc:
        return rc
    text = out_blob.tobytes()
    return [(text[b:e], int(parent), int(cb), int(cn), [c for c in range(16) if mask >> c & 1])
            for b, e, parent, cb, cn, mask in nodes[:n.value].tolist()], root_n.value


def cxx_walk(lib, ref, msg, columns):
    blob, key_lens, path_lens, kinds = c_columns(columns)
    tape = np.ascontiguousarray(ref.tape, dtype=np.uint64)
    strings = np.ascontiguousarray(np.append(ref.strings, np.uint8(0)))
    m = np.frombuffer(bytes(msg) + b"\0", dtype=np.uint8)
    cap = 4096
    out = np.zeros((cap, len(columns)), dtype=np.uint64)
    n = C.c_size_t(0)
    rc = lib.sj_selftest_table_walk(tape.ctypes.data, tape.size, strings.ctypes.data, m.ctypes.data, blob, key_lens.ctypes.data,
                                    path_lens.ctypes.data, kinds.ctypes.data, len(columns), out.ctypes.data, cap, C.byref(n))
    assert rc == 0 and n.value <= cap
    return out[:n.value].tolist()


def test_plan_has_the_same_nodes_in_the_same_order(cxx):
    for name, _, columns in CASES + [("random", None, RANDOM_COLUMNS)]:
        assert cxx_plan(cxx, columns) == TW.plan(columns), name
    # a parent in front of its children, the children of a node next to each other
    nodes, root_n = cxx_plan(cxx, DEEP_COLUMNS)
    assert root_n == 3 and len(nodes) == 18
    for j, (_, parent, cb, cn, _) in enumerate(nodes):
        assert parent == TW.ROOT or parent < j
        assert all(nodes[ch][1] == j for ch in range(cb, cb + cn)) and (cn == 0 or cb > j)


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_walk_replayed_over_the_oracles_tape(cxx, copy):
    for name, doc, columns in CASES:
        w, ref, msg = parsed(doc, copy)
        assert cxx_walk(cxx, ref, msg, columns) == TW.indexes(w, columns), name
    w, ref, msg = random_parsed(copy)
    got = cxx_walk(cxx, ref, msg, RANDOM_COLUMNS)
    assert len(got) == 3000 and got == TW.indexes(w, RANDOM_COLUMNS)
    # ... and against FindElement itself, column by column
    for c, (path, _) in enumerate(RANDOM_COLUMNS):
        assert [row[c] for row in got] == [w.find_path(root, list(path)) for root in w.records()], path


K = (b"k",)
LIMITS = [  # (columns, the refusal or 0)
    ([], TW.ERR_COLS), ([(K, I)] * 17, TW.ERR_COLS), ([(K, I)] * 16, 0), ([(K, I)], 0),
    ([(K, 6)], TW.ERR_KIND), ([(K, -1)], TW.ERR_KIND), ([(K, SC)], 0), ([(K, I), (K, 9)], TW.ERR_KIND),
    ([(K, I), ((), I)], TW.ERR_EMPTY_PATH),
    ([(K * 17, I)], TW.ERR_PATH_KEYS), ([(K * 16, I)], 0),
    ([(K * 16, I), (K * 16, S), (K, I)], TW.ERR_KEYS), ([(K * 16, I), (K * 16, S)], 0), ([(K * 2, I)] * 16, 0),
    ([((b"x" * 1024,), I), ((b"",), I)], 0), ([((b"x" * 1024,), I), ((b"y",), I)], TW.ERR_BYTES),
    ([((b"x" * 512, b"x" * 513), I)], TW.ERR_BYTES), ([((b"x" * 512, b"x" * 512), I)], 0),
]


def test_limits(cxx):
    for columns, want in LIMITS:
        got = cxx_plan(cxx, columns)
        if want:
            assert got == want, (columns[:2], len(columns))
            with pytest.raises(TW.Refused) as e:
                TW.plan(columns)
            assert e.value.code == want
        else:
            assert got == TW.plan(columns), (columns[:2], len(columns))
