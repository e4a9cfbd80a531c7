"""CPU: the restated array conversions of tests/list_walk.py (the checker of the device list columns), pinned three ways: a table of
small documents with the outputs written out by hand from parsed_array.go:145-344; on one-element arrays over the number texts of
tests/number_cases.py, agreement with column_walk.convert (Iter.Float / Int / Uint) everywhere but at the documented differences;
and CPython's int() / float() as the outside arbiter for the values in range."""
import column_walk as CW
import list_walk as LW
import number_cases as NC
import oracle_lib as O
import query_walk as Q

OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)
F, I, U = LW.COL_FLOAT, LW.COL_INT, LW.COL_UINT
fb = CW.f2bits
M63 = 1 << 63


def walk_of(doc, nd=False, copy=True):
    ref = O.parse(doc, ndjson=nd, copy_strings=copy)
    assert ref.rc == 0, doc
    return Q.Walk(ref.tape, ref.strings, doc[ref.msg_off:ref.msg_off + ref.msg_len])


def neg(x):
    return x & CW.U64


# document, path -> {kind: (status, values)}, "s": (status, [texts]) of AsString, "c": of AsStringCvt
A = (b"a",)
TABLE = [
    # the three number tags convert into each other; a uint above MaxInt64 fails AsInteger only
    (b'{"a":[1,2.5,18446744073709551615]}', A,
     {F: (OK, [fb(1.0), fb(2.5), fb(2.0 ** 64)]), I: (RANGE, []), U: (OK, [1, 2, (1 << 64) - 1]), "s": (TYPE, []),
      "c": (OK, [b"1", b"2.5", b"18446744073709551615"])}),
    (b'{"a":[-3,-2.75,7]}', A,
     {F: (OK, [fb(-3.0), fb(-2.75), fb(7.0)]), I: (OK, [neg(-3), neg(-2), 7]), U: (RANGE, []), "s": (TYPE, []),
      "c": (OK, [b"-3", b"-2.75", b"7"])}),
    # the empty array: OK with no elements, for every conversion
    (b'{"a":[]}', A, {F: (OK, []), I: (OK, []), U: (OK, []), "s": (OK, []), "c": (OK, [])}),
    # null at the path / inside the array
    (b'{"a":null}', A, {F: (NULL, []), I: (NULL, []), U: (NULL, []), "s": (NULL, []), "c": (NULL, [])}),
    (b'{"a":[null]}', A, {F: (TYPE, []), I: (TYPE, []), U: (TYPE, []), "s": (TYPE, []), "c": (OK, [b"null"])}),
    (b'{"a":[1,null]}', A, {F: (TYPE, []), I: (TYPE, []), U: (TYPE, []), "s": (TYPE, []), "c": (OK, [b"1", b"null"])}),
    # any other element at the path that is not an array
    (b'{"a":5}', A, {F: (TYPE, []), I: (TYPE, []), U: (TYPE, []), "s": (TYPE, []), "c": (TYPE, [])}),
    (b'{"a":"s"}', A, {F: (TYPE, []), "s": (TYPE, []), "c": (TYPE, [])}),
    (b'{"a":{"a":[1]}}', A, {F: (TYPE, []), "s": (TYPE, []), "c": (TYPE, [])}),
    (b'{"a":true}', A, {I: (TYPE, []), "c": (TYPE, [])}),
    # FindElement's errors
    (b'{"b":[1]}', A, {F: (NOT_FOUND, []), I: (NOT_FOUND, []), U: (NOT_FOUND, []), "s": (NOT_FOUND, []), "c": (NOT_FOUND, [])}),
    (b'[1,2]', A, {F: (NOT_OBJECT, []), I: (NOT_OBJECT, []), U: (NOT_OBJECT, []), "s": (NOT_OBJECT, []), "c": (NOT_OBJECT, [])}),
    (b'[{"a":[1]}]', A, {F: (NOT_OBJECT, []), "s": (NOT_OBJECT, [])}),
    (b'{"a":{"b":[1,2]}}', (b"a", b"b"), {F: (OK, [fb(1.0), fb(2.0)]), I: (OK, [1, 2]), U: (OK, [1, 2]), "c": (OK, [b"1", b"2"])}),
    (b'{"a":{"b":[1,2]}}', (b"a", b"b", b"c"), {F: (NOT_OBJECT, []), "s": (NOT_OBJECT, [])}),
    (b'{"a":[7],"a":[8]}', A, {I: (OK, [7])}),  # the first member with the key wins
    # the first failing element decides: a RANGE before a TYPE, and the reverse
    (b'{"a":[-1,"x"]}', A, {U: (RANGE, []), I: (TYPE, []), F: (TYPE, [])}),
    (b'{"a":["x",-1]}', A, {U: (TYPE, []), I: (TYPE, [])}),
    (b'{"a":[9223372036854775808,true]}', A, {I: (RANGE, []), U: (TYPE, [])}),
    (b'{"a":[true,9223372036854775808]}', A, {I: (TYPE, []), U: (TYPE, [])}),
    (b'{"a":[1e300,null]}', A, {I: (RANGE, []), U: (RANGE, []), F: (TYPE, [])}),
    (b'{"a":[null,1e300]}', A, {I: (TYPE, []), U: (TYPE, []), F: (TYPE, [])}),
    # the edges at 2^63, -2^63, -0.0 and 2^64
    (b'{"a":[9223372036854775808.0]}', A, {F: (OK, [fb(2.0 ** 63)]), I: (OK, [M63]), U: (OK, [M63])}),
    (b'{"a":[-9223372036854775808.0]}', A, {F: (OK, [fb(-(2.0 ** 63))]), I: (OK, [M63]), U: (RANGE, [])}),
    (b'{"a":[9223372036854777856.0]}', A, {I: (RANGE, []), U: (RANGE, [])}),  # 2^63 + 2048, the next double
    (b'{"a":[-9223372036854777856.0]}', A, {I: (RANGE, []), U: (RANGE, [])}),
    (b'{"a":[-0.0]}', A, {F: (OK, [M63]), I: (OK, [0]), U: (OK, [0]), "c": (OK, [b"-0"])}),
    (b'{"a":[18446744073709551616.0]}', A, {F: (OK, [fb(2.0 ** 64)]), I: (RANGE, []), U: (RANGE, [])}),  # (Iter.Uint: OK, 0)
    (b'{"a":[9223372036854775807,9223372036854775808]}', A, {I: (RANGE, []), U: (OK, [M63 - 1, M63])}),
    (b'{"a":[-9223372036854775808]}', A, {I: (OK, [M63]), U: (RANGE, []), F: (OK, [fb(-(2.0 ** 63))])}),
    # nested containers are elements no conversion accepts
    (b'{"a":[[1],[2]]}', A, {F: (TYPE, []), I: (TYPE, []), U: (TYPE, []), "s": (TYPE, []), "c": (TYPE, [])}),
    (b'{"a":[1,[2]]}', A, {F: (TYPE, []), "c": (TYPE, [])}),
    (b'{"a":["x",{"a":1}]}', A, {"s": (TYPE, []), "c": (TYPE, [])}),
    # strings
    (b'{"a":["x","","caf\\u00e9","q\\"\\n"]}', A,
     {"s": (OK, [b"x", b"", "café".encode(), b'q"\n']), "c": (OK, [b"x", b"", "café".encode(), b'q"\n']), F: (TYPE, [])}),
    (b'{"a":["x",1]}', A, {"s": (TYPE, []), "c": (OK, [b"x", b"1"])}),
    (b'{"a":[true,false,null,1.5,-3,"s",1e21,1e-7]}', A,
     {"s": (TYPE, []), "c": (OK, [b"true", b"false", b"null", b"1.5", b"-3", b"s", b"1e+21", b"1e-7"])}),
]


def test_table_of_small_documents():
    seen = {k: set() for k in (F, I, U, "s", "c")}
    for doc, path, want in TABLE:
        for copy in (True, False):
            w = walk_of(doc, copy=copy)
            (root,) = w.records()
            v, st = LW.array_at(w, root, path)
            for kind, (want_st, want_v) in want.items():
                if kind in (F, I, U):
                    got = (st, []) if v is None else LW.NUMERIC[kind](w, v)
                    col = LW.list_column(w, path, kind)
                    assert col == ([0, len(want_v)], want_v, [want_st]), (doc, kind, col)
                else:
                    got = (st, []) if v is None else LW._texts(w, v, kind == "c")
                    col = LW.list_string_column(w, path, kind == "c")
                    so = [0]
                    for b in want_v:
                        so.append(so[-1] + len(b))
                    assert col == ([0, len(want_v)], so, b"".join(want_v), [want_st]), (doc, kind, col)
                assert got == (want_st, want_v), (doc, kind, got)
                seen[kind].add(want_st)
    for kind in (F, I, U):
        assert seen[kind] >= ({OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL} | ({RANGE} if kind != F else set())), (kind, seen[kind])
    assert seen["s"] >= {OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL} and seen["c"] >= {OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL}


def test_layout_over_records():
    doc = b'{"a":[1,2]}\n{"a":null}\n{"a":[]}\n{"b":0}\n{"a":["x",3]}\n{"a":[4]}\n[5]'
    w = walk_of(doc, nd=True)
    assert LW.list_column(w, A, I) == ([0, 2, 2, 2, 2, 2, 3, 3], [1, 2, 4], [OK, NULL, OK, NOT_FOUND, TYPE, OK, NOT_OBJECT])
    assert LW.list_string_column(w, A, True) == ([0, 2, 2, 2, 2, 4, 5, 5], [0, 1, 2, 3, 4, 5], b"12x34",
                                                 [OK, NULL, OK, NOT_FOUND, OK, OK, NOT_OBJECT])
    assert LW.list_string_column(w, A, False) == ([0] * 8, [0], b"", [TYPE, NULL, OK, NOT_FOUND, TYPE, TYPE, NOT_OBJECT])


# ---- one-element arrays over the arbiter's number texts: hand-made tapes {"k":[x]} ---------------------------------------------
def one_element(tag_word, raw):
    T = lambda c, p=0: (ord(c) << 56) | p
    t = [T("r", 10), T("{", 9), T('"', Q.STRINGBUFBIT), 1, T("[", 8), tag_word, raw, T("]", 4), T("}", 1), T("r", 0)]
    return Q.Walk(t, b"k", b"")


def test_agrees_with_the_scalar_conversions_and_cpython_on_the_number_cases():
    n = diffs = 0
    for name, cases in NC.families().items():
        cases = NC.accepted(cases)
        if name == "random_fill":
            cases = cases[::40]
        for text, exp in cases:
            w = one_element(*NC.words(exp))
            (root,) = w.records()
            v, st = LW.array_at(w, root, [b"k"])
            assert (v, st) == (4, OK)
            d = NC.as_double(exp)
            for kind in (F, I, U):
                got = LW.NUMERIC[kind](w, v)
                scalar_st, scalar_x = CW.convert(w, 5, kind)
                if kind == U and exp[0] == "d" and 2.0 ** 63 < d <= 2.0 ** 64:
                    assert got == (RANGE, []) and scalar_st == OK, text  # parsed_array.go:253 against parsed_json.go:685
                    diffs += 1
                else:
                    assert got == ((OK, [scalar_x]) if scalar_st == OK else (scalar_st, [])), (text, kind, got)
                # CPython as the arbiter of the values in range
                if kind == F:
                    assert got == (OK, [fb(float(text) if exp[0] == "d" else float(int(text)))]), text  # ("-0" is the integer 0)
                elif exp[0] != "d":
                    lo, hi = (-(1 << 63), 1 << 63) if kind == I else (0, 1 << 64)
                    assert got == ((OK, [int(text) & CW.U64]) if lo <= int(text) < hi else (RANGE, [])), (text, kind)
                elif (kind == I and abs(d) < 2.0 ** 63) or (kind == U and 0.0 <= d < 2.0 ** 63):
                    assert got == (OK, [int(float(text)) & CW.U64]), (text, kind)
            n += 1
    assert n > 20000 and diffs > 0, (n, diffs)
    # the other documented difference: a null element is a type error for the array, NULL for Iter.Float / Int / Uint
    w = walk_of(b'{"k":[null]}')
    (root,) = w.records()
    v, _ = LW.array_at(w, root, [b"k"])
    for kind in (F, I, U):
        assert LW.NUMERIC[kind](w, v) == (TYPE, []) and CW.convert(w, v + 1, kind) == (NULL, 0)
