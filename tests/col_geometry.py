"""The cuts of the string column and of the list columns (k_q_col_len / k_q_col_gather, k_q_list_measure[_cvt], the scans of
n + 1 entries, k_q_list_gather_num / _str / _cvt, csrc/query.hip), restated -- the geometry, the case builders and a host model
(test infrastructure, like batch_geometry.py and agg_geometry.py).  column_walk.py and list_walk.py say WHAT a column is; this
file says which lane, wave, step, scan tile and block gets there, so that a case can prove it lies on the cut it is named for.

Geometry.  One thread per record in blocks of BLOCK = 256, waves of WAVE = 64:
  string_route(len)          a string of up to COL_SHORT = 32 bytes is copied by its record's lane, a longer one by the whole wave
                             in steps of 64 bytes -> (route, steps)
  list_measure_route(words)  k_q_list_measure sends an array to the wave by the WORDS between its brackets (> 2 * LIST_SHORT)
  list_gather_route(elems)   the gathers by its ELEMENTS (> LIST_SHORT = 16); AsStringCvt arrays are always their lane's
  steps(elems)               wave steps of 64 elements
  scan_tiles(n)              the tiles (QTILE = QT * QI = 1024) of the n + 1 entries of a length array (tiles_of)
  measure_blocks(n)          (n + 1 + 255) / 256: entry n is written by thread n -- in a block of its own when n % 256 == 0
  gather_blocks(n)           (n + 255) / 256

Builders.  A record is described by elements (El): its JSON text, its tape words and what every conversion makes of it.  Strings
carry bytes that depend on (row, element, byte index), numbers are 1000 * row + k, so a byte or an element one slot off differs
from its neighbour.  expect(case, mode) derives offsets, values or bytes, statuses and totals from that description alone --
neither the walkers nor the tape are asked.  Case(name, family, doc, path, select, rows, claim, debug): claim[r] says what the
model's trace must show for row r (route, steps, the failing ballot, the rounds of waiting lanes); debug: the case also runs on
the bounds-checked build.

The host model.  model(doc, path, mode, **mutations) walks the oracle's tape the way the three kernels do -- measure with a route
per record, wave steps, one ballot and its lowest lane, entry n; the tiled scan; the gather with its lane copies, wave copies, the
wait-and-copy rounds and AsString's carried base -- and returns the arrays a fetch would deliver plus a trace.  What no lane
writes stays POISON.  MUTATIONS names one deliberate mistake each; a threshold mutation moves one side of a cut only (the lane's
test or the wave's), because a kernel that moves both still fetches the same arrays.  tests/test_col_geometry.py shows which case
tells every mutation from the kernels; tests/test_gpu_column_seams.py runs the cases on the device."""
import collections
import functools

import column_walk as CW
import list_walk as LW
import oracle_lib as O
import query_walk as Q
import rows_walk as RW

COL_SHORT, LIST_SHORT = 32, 16
WAVE, BLOCK = 64, 256
QT, QI = 256, 4
QTILE = QT * QI
OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)
FLOAT, INT, UINT = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT
U64 = (1 << 64) - 1
LANE, WIDE = "lane", "wave"
MODES = {"strings": ("strings", "strings_cvt"), "numbers": ("float", "int", "uint"), "list_strings": ("list_str", "list_cvt")}
KIND = {"float": FLOAT, "int": INT, "uint": UINT}
RAW = {"[": 6557241057451442176, "{": 8863084066665136128, "]": 6701356245527298048, "}": 9007199254740992000,
       "l": 7782220156096217088, '"': 2449958197289549824}  # integers whose top byte is a tag (tests/test_gpu_rows.py)


# ---- the cuts -------------------------------------------------------------------------------------------------------------------------
def string_route(n):
    return (LANE, 0) if n <= COL_SHORT else (WIDE, (n + WAVE - 1) // WAVE)


def list_measure_route(words):
    return WIDE if words > 2 * LIST_SHORT else LANE


def list_gather_route(elems):
    return WIDE if elems > LIST_SHORT else LANE


def steps(elems):
    return (elems + WAVE - 1) // WAVE


def scan_tiles(n):
    return (n + 1 + QTILE - 1) // QTILE


def measure_blocks(n):
    return (n + 1 + BLOCK - 1) // BLOCK


def gather_blocks(n):
    return (n + BLOCK - 1) // BLOCK


# ---- elements -------------------------------------------------------------------------------------------------------------------------
# text: the JSON text; words: its tape words; plain: the bytes Iter.StringBytes returns (None: not a string); cvt: the bytes
# StringCvt returns (None: a container); num: {kind: (status, bits)} of the Array conversions (None: a type error); st_plain: the
# status of StringBytes on it
El = collections.namedtuple("El", "text words plain cvt num st_plain")
ALPHA = bytes(c for c in range(0x21, 0x7F) if c not in b'"\\')[:89]  # (89 is prime)
_ALPHA = ALPHA * 8


def s_el(row, k, n, esc=False):
    """a string of n decoded bytes; esc: every eighth byte is a line feed, written as an escape (the raw text is longer)"""
    start = (37 * row + 11 * k) % 89
    body = (_ALPHA * (n // 600 + 1))[start:start + n]
    if not esc:
        return El('"%s"' % body.decode(), 2, body, body, None, TYPE)
    dec = bytes(0x0A if i % 8 == 3 else c for i, c in enumerate(body))
    return El('"%s"' % dec.replace(b"\n", b"\\n").decode(), 2, dec, dec, None, TYPE)


def n_el(v):
    """an integer in [0, 2^63): every kind accepts it"""
    assert 0 <= v < 1 << 63
    return El(str(v), 2, None, str(v).encode(), {FLOAT: (OK, CW.f2bits(float(v))), INT: (OK, v), UINT: (OK, v)}, TYPE)


def _num(text, f, i, u):
    return El(text, 2, None, text.encode(), {FLOAT: f, INT: i, UINT: u}, TYPE)


def box(text, words):
    return El(text, words, None, None, None, TYPE)


I64MIN = _num("-9223372036854775808", (OK, CW.f2bits(-2.0 ** 63)), (OK, 1 << 63), (RANGE, 0))
U64MAX = _num("18446744073709551615", (OK, CW.f2bits(2.0 ** 64)), (RANGE, 0), (OK, U64))
FLTMAX = _num("-2.2250738585072014e-308", (OK, CW.f2bits(-2.2250738585072014e-308)), (OK, 0), (RANGE, 0))  # 24 bytes of text
E300 = _num("1e300", (OK, CW.f2bits(1e300)), (RANGE, 0), (RANGE, 0))._replace(cvt=b"1e+300")
M1 = _num("-1", (OK, CW.f2bits(-1.0)), (OK, U64), (RANGE, 0))
M15 = _num("-1.5", (OK, CW.f2bits(-1.5)), (OK, U64), (RANGE, 0))  # (int64(-1.5) = -1)
TRUE = El("true", 1, None, b"true", None, TYPE)
FALSE = El("false", 1, None, b"false", None, TYPE)
NUL = El("null", 1, None, b"null", None, NULL)
EMPTY_ARR, ONE_ARR, OBJ12, EMPTY_OBJ = box("[]", 2), box("[1]", 4), box('{"a":[1,2,3]}', 12), box("{}", 2)
OBJ40 = box('{"a":[%s]}' % ",".join(str(k) for k in range(17)), 40)
LONGEST = (I64MIN, U64MAX, FLTMAX, TRUE, FALSE, NUL)

Case = collections.namedtuple("Case", "name family doc path select rows claim debug")


# ---- what the columns must be, from the description alone ---------------------------------------------------------------------------
def _expect_strings(rows, cvt):
    off, parts, st = [0], [], []
    for e in rows:
        b = b""
        if e is None:
            st.append(NOT_FOUND)
        else:
            b = e.cvt if cvt else e.plain
            st.append(OK if b is not None else e.st_plain)
            b = b or b""
        parts.append(b)
        off.append(off[-1] + len(b))
    return dict(off=off, data=b"".join(parts), status=st, totals=(len(rows), off[-1]))


def _not_array(a):
    return NOT_FOUND if a is None else (NULL if a is NUL else TYPE)


def _expect_numbers(rows, kind):
    off, vals, sts = [0], [], []
    for a in rows:
        st, xs = OK, []
        if not isinstance(a, list):
            st = _not_array(a)
        else:
            for e in a:
                st, x = e.num[kind] if e.num else (TYPE, 0)
                if st != OK:
                    xs = []
                    break
                xs.append(x)
        vals += xs
        off.append(len(vals))
        sts.append(st)
    return dict(off=off, vals=vals, status=sts, totals=(len(rows), len(vals)))


def _expect_list_strings(rows, cvt):
    off, soff, parts, sts = [0], [0], [], []
    for a in rows:
        st, bs = OK, []
        if not isinstance(a, list):
            st = _not_array(a)
        else:
            for e in a:
                b = e.cvt if cvt else e.plain
                if b is None:
                    st, bs = TYPE, []
                    break
                bs.append(b)
        for b in bs:
            parts.append(b)
            soff.append(soff[-1] + len(b))
        off.append(len(soff) - 1)
        sts.append(st)
    return dict(off=off, soff=soff, data=b"".join(parts), status=sts, totals=(len(rows), len(soff) - 1, soff[-1]))


@functools.lru_cache(maxsize=None)
def _expect(name, mode):
    c = CASES[name]
    if mode in ("strings", "strings_cvt"):
        return _expect_strings(c.rows, mode == "strings_cvt")
    if mode in KIND:
        return _expect_numbers(c.rows, KIND[mode])
    return _expect_list_strings(c.rows, mode == "list_cvt")


def expect(case, mode):
    return _expect(case.name, mode)


FIELDS = ("off", "soff", "vals", "data", "status", "totals")


def differing(got, want):
    """the fields in which two results differ"""
    return tuple(k for k in FIELDS if k in want and (k not in got or list(got[k]) != list(want[k])))


def differs(got, want):
    """the first field in which two results differ, or None"""
    return (differing(got, want) + (None,))[0]


# ---- documents ------------------------------------------------------------------------------------------------------------------------
def _value_text(v):
    return "[" + ",".join(e.text for e in v) + "]" if isinstance(v, list) else v.text


def _doc(rows, key, select=None):
    items = [('{"%s":%s}' % (key, _value_text(v))) if v is not None else '{"x":0}' for v in rows]
    if select is not None:
        return ('{"%s":[%s]}' % (select[0].decode(), ",".join(items))).encode()
    return "\n".join(items).encode()


def _words(v):
    return sum(e.words for e in v)


def walk(doc, copy=True, select=None):
    """the oracle's parse as a Walk; under a selection its rows stand in the place of the records"""
    ref = O.parse(doc, ndjson=True, copy_strings=copy)
    assert ref.rc == 0
    w = Q.Walk(ref.tape, ref.strings, doc[ref.msg_off:ref.msg_off + ref.msg_len])
    return RW.on_rows(w, select) if select is not None else w


def place(r):
    return dict(lane=r % WAVE, wave=r % BLOCK // WAVE, block=r // BLOCK, tile=r // QTILE)


# ---- the string column ----------------------------------------------------------------------------------------------------------------
STR_LENS = (0, 1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 32 + 3 * 64 + 1)
PLACES = (0, 1, 62, 63, 192, 193, 254, 255)  # lanes 0, 1, 62, 63 of wave 0 and of wave 3 of a block
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1022, 1023, 1024, 1025, 2047, 2048)
PARTIAL = (65, 127)  # 64 k + 1 and 64 k + 63


def _scase(name, rows, claim, select=None, debug=False):
    return Case(name, "strings", _doc(rows, "s", select), (b"s",), select, rows, claim, debug)


def _sclaim(rows, which):
    return {r: dict(route=string_route(len(rows[r].plain)), **place(r)) for r in which}


def string_cases():
    out = []
    for n in STR_LENS:
        rows = [s_el(r, 0, n if r in PLACES else r % 7) for r in range(BLOCK)]
        out.append(_scase("strings: %d bytes at lanes 0, 1, 62, 63 of waves 0 and 3" % n, rows, _sclaim(rows, PLACES)))
    rows = [s_el(r, 0, 33 + 3 * r) for r in range(WAVE)]
    out.append(_scase("strings: a wave of 64 wide strings", rows, _sclaim(rows, range(WAVE))))
    rows = [s_el(r, 0, 129 if r in (0, 63) else r % 9) for r in range(WAVE)]
    out.append(_scase("strings: only lanes 0 and 63 wide", rows, _sclaim(rows, range(WAVE))))
    rows = [s_el(r, 0, 33 + r if r % 2 else r % 5) for r in range(WAVE)]
    out.append(_scase("strings: wide and short strings alternate", rows, _sclaim(rows, range(WAVE))))
    for n in PARTIAL:
        rows = [s_el(r, 0, r % 11) for r in range(n - 1)] + [s_el(n - 1, 0, 129)]
        out.append(_scase("strings: %d rows, the last one wide in a partial wave" % n, rows, _sclaim(rows, [n - 1]), debug=True))
    for n in COUNTS:
        rows = [s_el(r, 0, 97 if r in (QTILE - 1, QTILE) else 7 * r % 40) for r in range(n)]
        out.append(_scase("strings: %d rows" % n, rows, _sclaim(rows, [r for r in (QTILE - 1, QTILE, n - 1) if r < n])))
    rows = []
    for k, e in enumerate(LONGEST):
        rows += [s_el(2 * k, 0, 65 + k), e]
    rows.append(s_el(99, 0, 70))
    out.append(_scase("strings: the longest number texts and the literals between wide strings", rows,
                      _sclaim(rows, range(0, len(rows), 2))))
    rows = []
    for r, n in enumerate((32, 33, 64, 65, 31, 63)):
        rows += [s_el(3 * r, 0, n, esc=True), s_el(3 * r + 1, 0, r), s_el(3 * r + 2, 0, n)]
    out.append(_scase("strings: escapes, decoded 32 / 33 / 64 / 65 bytes from a longer text", rows, _sclaim(rows, range(0, len(rows), 3))))
    rows = [s_el(r, 0, r % 13) for r in range(256)] + [s_el(256, 0, 129)]
    out.append(_scase("strings: 257 selected rows, the last one wide", rows, _sclaim(rows, [256]), select=(b"items",), debug=True))
    return out


# ---- numeric lists --------------------------------------------------------------------------------------------------------------------
LIST_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 80, 127, 128, 129, 192, 193)
FAIL_E = (16, 17, 64, 65, 129, 200)
FAIL_F = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128)
FAIL_AT = [(e, f) for e in FAIL_E for f in sorted(set(ff for ff in FAIL_F + (e - 1,) if ff < e))]


def nums(r, n, first=0):
    return [n_el(1000 * r + k) for k in range(first, first + n)]


def _ncase(name, rows, claim, debug=False):
    return Case(name, "numbers", _doc(rows, "a"), (b"a",), None, rows, claim, debug)


def _fail_at(a, kind):
    """index of the first element the conversion refuses, or None"""
    for k, e in enumerate(a):
        if (e.num[kind][0] if e.num else TYPE) != OK:
            return k
    return None


def _nclaim(rows, which):
    out = {}
    for r in which:
        a = rows[r]
        c = dict(measure=list_measure_route(_words(a)), **place(r))
        for mode, kind in KIND.items():
            f = _fail_at(a, kind)
            c["gather@" + mode] = list_gather_route(len(a) if f is None else 0)
            c["fail@" + mode] = None if f is None else (f if c["measure"] == LANE else (f // WAVE, f % WAVE))
        out[r] = c
    return out


def _with(a, f, e):
    return a[:f] + [e] + a[f + 1:]


def number_cases():
    out = []
    for n in LIST_LENS:
        rows = [nums(r, n if r in (0, 63) else r % 4) for r in range(WAVE)]
        rows[5], rows[6], rows[7] = NUL, None, TRUE  # (null, no such key and a scalar at the path own no elements)
        out.append(_ncase("numbers: %d elements at lanes 0 and 63" % n, rows, _nclaim(rows, (0, 63))))
    rows = [nums(r, 17 + r % 3) for r in range(WAVE)]
    out.append(_ncase("numbers: a wave of 64 wide arrays", rows, _nclaim(rows, range(WAVE))))
    for n in PARTIAL:
        rows = [nums(r, r % 5) for r in range(n - 1)] + [nums(n - 1, 129)]
        out.append(_ncase("numbers: %d rows, the last array wide in a partial wave" % n, rows, _nclaim(rows, [n - 1]), debug=True))
    for n in COUNTS:
        rows = [nums(r, 5 * r % 19) for r in range(n)]
        out.append(_ncase("numbers: %d rows" % n, rows, _nclaim(rows, [r for r in (QTILE - 1, QTILE, n - 1) if r < n])))
    rows = [nums(r, 1025 if r == QTILE - 1 else 1) for r in range(QTILE + 1)]
    out.append(_ncase("numbers: 1025 elements in the last entry of a scan tile", rows, _nclaim(rows, [QTILE - 1, QTILE])))
    fails = [("a string", lambda r: s_el(r, 0, 3)), ("null", lambda r: NUL), ("[]", lambda r: EMPTY_ARR), ("[1]", lambda r: ONE_ARR),
             ("an object", lambda r: OBJ12), ("1e300", lambda r: E300), ("-1", lambda r: M1)]
    for what, el in fails:
        rows = [_with(nums(r, e), f, el(r)) for r, (e, f) in enumerate(FAIL_AT)]
        out.append(_ncase("numbers: first failing element %s at every (E, f)" % what, rows, _nclaim(rows, range(len(rows))), debug=True))
    for what, tags in (("l", "l"), ("every tag", '[{]}l"')):  # behind the one-word element every shifted read sees a tag
        rows = [nums(r, f) + [TRUE] + [n_el(RAW[tags[k % len(tags)]]) for k in range(e - f - 1)] for r, (e, f) in enumerate(FAIL_AT)]
        out.append(_ncase("numbers: true at every (E, f), payloads that look like %s behind it" % what, rows,
                          _nclaim(rows, range(len(rows))), debug=True))
    a = nums(0, 65)
    rows = [_with(_with(a, 3, s_el(0, 3, 2)), 40, M15), _with(_with(a, 3, M15), 40, s_el(1, 40, 2)),  # TYPE | RANGE for UINT, in one step
            _with(_with(a, 0, E300), 63, NUL), _with(_with(a, 0, NUL), 63, E300),
            _with(_with(nums(4, 200), 10, s_el(4, 10, 1)), 70, M1), _with(_with(nums(5, 200), 10, M1), 70, s_el(5, 70, 1)),  # two steps
            _with(_with(nums(6, 200), 63, E300), 64, NUL), _with(_with(nums(7, 200), 127, NUL), 128, E300)]
    out.append(_ncase("numbers: two failures of different status, in one step and in two, both orders", rows, _nclaim(rows, range(len(rows))),
                      debug=True))
    rows = [nums(r, r % 4) for r in range(WAVE)]
    rows[0] = nums(0, 15) + [ONE_ARR]          # 34 words, 16 elements
    rows[1], rows[2] = nums(1, 16), nums(2, 17)  # 32 words next to 34
    rows[3] = _with(nums(3, 3), 1, OBJ40)      # 44 words, 3 elements
    rows[4] = nums(4, 16) + [TRUE]             # 33 words: an odd count above the cut
    rows[62] = [ONE_ARR] + nums(62, 15)
    rows[63] = nums(63, 15) + [ONE_ARR]
    out.append(_ncase("numbers: words say wave, elements say lane", rows, _nclaim(rows, (0, 1, 2, 3, 4, 62, 63)), debug=True))
    return out


# ---- string lists ---------------------------------------------------------------------------------------------------------------------
LSTR_LENS = (0, 1, 32, 33, 64, 65, 200)


def strs(r, n, length):
    """n strings; length: a number or a function of the element index"""
    return [s_el(r, k, length(k) if callable(length) else length) for k in range(n)]


def _lcase(name, rows, claim, debug=False):
    return Case(name, "list_strings", _doc(rows, "t"), (b"t",), None, rows, claim, debug)


def _lclaim(rows, which, rounds=None):
    out = {}
    for r in which:
        a = rows[r]
        c = dict(place(r))
        plain = all(e.plain is not None for e in a)
        c["measure@list_str"] = list_measure_route(_words(a))
        c["gather@list_str"] = list_gather_route(len(a) if plain else 0)
        c["gather@list_cvt"] = LANE
        if plain and len(a) > LIST_SHORT:
            c["long@list_str"] = [(k // WAVE, k % WAVE) for k, e in enumerate(a) if len(e.plain) > COL_SHORT]
        out[r] = c
    if rounds is not None:
        out["rounds"] = rounds
    return out


def _rounds(rows, cvt):
    """the waiting lanes of every round of the wait-and-copy loop, per wave, from the description"""
    out = {}
    for base in range(0, len(rows), WAVE):
        waits = {}
        for lane, a in enumerate(rows[base:base + WAVE]):
            if not isinstance(a, list) or any((e.cvt if cvt else e.plain) is None for e in a) or (not cvt and len(a) > LIST_SHORT):
                continue
            n = sum(1 for e in a if e.plain is not None and len(e.plain) > COL_SHORT)
            for k in range(n):
                waits.setdefault(k, []).append(lane)
        out[base // WAVE] = [tuple(waits[k]) for k in sorted(waits)]
    return out


def _wait_claim(rows, which):
    c = _lclaim(rows, which)
    c["rounds@list_str"], c["rounds@list_cvt"] = _rounds(rows, False), _rounds(rows, True)
    return c


def list_string_cases():
    out = []
    for n in LSTR_LENS:
        rows = [strs(r, r % 3, r % 5) for r in range(WAVE)]
        for r, e in enumerate(LIST_LENS):
            rows[r] = strs(r, e, n)
        rows[63] = strs(63, 65, n)
        out.append(_lcase("list strings: every element count with strings of %d bytes" % n, rows, _wait_claim(rows, list(range(14)) + [63])))
    long_at = lambda at: (lambda k: 70 + at if k == at else k % 4)  # noqa: E731
    rows = [strs(r, r % 4, r % 6) for r in range(WAVE)]
    rows[3], rows[4], rows[5] = strs(3, 5, long_at(0)), strs(4, 5, long_at(2)), strs(5, 5, long_at(4))
    out.append(_lcase("list strings: a long string first, in the middle and last in a short array", rows, _wait_claim(rows, (3, 4, 5))))
    rows = [strs(r, r % 4, r % 6) for r in range(WAVE)]
    rows[5], rows[9] = strs(5, 2, long_at(0)), strs(9, 3, long_at(0))
    out.append(_lcase("list strings: two lanes wait in the same round", rows, _wait_claim(rows, (5, 9))))
    rows = [strs(r, r % 4, r % 6) for r in range(WAVE)]
    rows[7] = strs(7, 3, lambda k: 0 if k == 1 else 40 + k)  # waits at elements 0 and 2
    rows[8] = strs(8, 3, lambda k: 90 if k == 1 else 2)      # waits at element 1
    rows[20] = strs(20, 4, lambda k: 50 if k == 3 else 1)    # joins the first round from its last element
    out.append(_lcase("list strings: lanes wait in different rounds", rows, _wait_claim(rows, (7, 8, 20))))
    rows = [strs(r, r % 4, r % 6) for r in range(WAVE)]
    rows[31] = strs(31, 16, lambda k: 33 + 9 * k)
    out.append(_lcase("list strings: one lane with 16 long strings, 63 lanes with none", rows, _wait_claim(rows, (31,))))
    rows = [strs(r, r % 4, r % 6) for r in range(WAVE)]
    rows[0], rows[63] = strs(0, 3, lambda k: 64 + k), strs(63, 2, lambda k: 129 - k)
    out.append(_lcase("list strings: the waiting lanes are 0 and 63", rows, _wait_claim(rows, (0, 63))))
    for n in PARTIAL:
        rows = [strs(r, r % 4, r % 6) for r in range(n - 2)] + [strs(n - 2, 4, lambda k: 40 * k), strs(n - 1, 65, lambda k: 129 if k % 32 == 0 else k % 3)]
        out.append(_lcase("list strings: %d rows, a waiting lane and a wide array in a partial wave" % n, rows, _wait_claim(rows, (n - 2, n - 1)),
                          debug=True))
    rows = [strs(r, r % 4, r % 6) for r in range(WAVE)]
    for r, e in enumerate((64, 65, 128, 129)):
        rows[r] = strs(r, e, lambda k: 65 + k % 7 if k % WAVE in (0, 63) else k % 5)
    rows[4] = strs(4, 129, lambda k: 0 if WAVE <= k < 2 * WAVE else 3)  # a step of only empty strings
    rows[5] = strs(5, 128, 0)
    rows[63] = strs(63, 129, lambda k: 200 if k % WAVE in (0, 63) else 0)
    out.append(_lcase("list strings: AsString steps that end at 64 and 128, long strings at lanes 0 and 63 of a step", rows,
                      _wait_claim(rows, (0, 1, 2, 3, 4, 5, 63))))
    rows = [strs(r, r % 4, r % 6) for r in range(WAVE)]
    for r, e in enumerate((17, 65, 130)):
        mix = [LONGEST[k % 6] if k % 3 == 0 else s_el(r, k, 97 if k % 16 == 1 else k % 4) if k % 3 == 1 else n_el(1000 * r + k) for k in range(e)]
        rows[r] = rows[61 + r] = mix
    out.append(_lcase("list strings: AsStringCvt arrays of 17, 65 and 130 one-word and two-word elements", rows, _wait_claim(rows, (0, 1, 2, 61, 62, 63))))
    for what, el in (("a number", lambda r: n_el(1000 * r)), ("{}", lambda r: EMPTY_OBJ), ("[]", lambda r: EMPTY_ARR)):
        rows = [_with(strs(r, e, lambda k: 40 if k % 50 == 7 else k % 5), f, el(r)) for r, (e, f) in enumerate(FAIL_AT)]
        out.append(_lcase("list strings: %s at every (E, f)" % what, rows, _wait_claim(rows, range(len(rows))), debug=True))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(string_cases() + number_cases() + list_string_cases())


class _Cases(dict):
    def __missing__(self, name):
        self.update({c.name: c for c in all_cases()})
        return dict.__getitem__(self, name)


CASES = _Cases()


# ---- the host model -------------------------------------------------------------------------------------------------------------------
POISON, POISON_V, JUNK = 0xA5, 0xA5A5A5A5A5A5A5A5, 7  # a byte nobody wrote; a value nobody wrote; what an unwritten entry n holds
MUTATIONS = {
    "COL_SHORT - 1 in the lane's test": dict(col_lane=COL_SHORT - 1),
    "COL_SHORT + 1 in the wave's test": dict(col_wave=COL_SHORT + 1),
    "LIST_SHORT - 1 in the lane's test": dict(list_lane=LIST_SHORT - 1),
    "LIST_SHORT + 1 in the wave's test": dict(list_wave=LIST_SHORT + 1),
    "a wave step of 63": dict(step=63),
    "entry n not written": dict(entry_n=False),
    "the highest failing lane": dict(highest=True),
    "shifted words trusted behind a one-word element": dict(trust_shifted=True),
    "the measure routed by elements": dict(by_elems=True),
    "base not carried between AsString steps": dict(carry=False),
    "the lanes without a record left out of the step loop": dict(recordless=False),
}
_DEFAULTS = dict(col_lane=COL_SHORT, col_wave=COL_SHORT, list_lane=LIST_SHORT, list_wave=LIST_SHORT, step=WAVE, entry_n=True, highest=False,
                 trust_shifted=False, by_elems=False, carry=True, recordless=True)
_K = collections.namedtuple("_K", sorted(_DEFAULTS))


def _tag(w, p):
    return chr(w.t[p] >> 56)


def _scan(a):
    """tile sums -> their exclusive prefix -> apply, over all entries; -> (exclusive prefix, the total the call reports)"""
    sums = [sum(a[t:t + QTILE]) for t in range(0, len(a), QTILE)]
    out, acc = [], 0
    for t, s in enumerate(sums):
        pre = acc
        for x in a[t * QTILE:(t + 1) * QTILE]:
            out.append(pre)
            pre += x
        acc += s
    return out, acc


def _waves(threads, n, K):
    """(first thread, the lanes with a record, the lanes that run the wave's loops) of every wave of a launch"""
    for base in range(0, threads, WAVE):
        active = [l for l in range(WAVE) if base + l < n]
        yield base, active, (list(range(WAVE)) if K.recordless else active)


def _wave_copy(data, wide, workers, K):
    """wave_copy_strings: the strings {lane: (offset, length, bytes)} one after another, byte k by lane k % 64"""
    for j in sorted(wide):
        o, ln, src = wide[j]
        for lane in workers:
            data[o + lane:o + ln:K.step] = src[lane:ln:K.step]


def _measure_threads(n, K):
    return (measure_blocks(n) if K.entry_n else gather_blocks(n)) * BLOCK  # (without the + 1 thread n exists unless n % 256 == 0)


def _model_strings(w, path, cvt, K):
    recs = w.records()
    n = len(recs)
    idx, ln, st = [0] * n, [JUNK] * (n + 1), [0] * n
    for r in range(min(_measure_threads(n, K), n + 1)):  # k_q_col_len
        if r == n:
            ln[n] = 0
            break
        v = w.find_path(recs[r], list(path))
        if v >= Q.NOT_OBJECT:
            st[r], ln[r] = (NOT_OBJECT if v == Q.NOT_OBJECT else NOT_FOUND), 0
        else:
            st[r], b = CW.text(w, v, cvt)
            idx[r], ln[r] = v, len(b)
    off, total = _scan(ln)
    data = bytearray([POISON]) * total
    out_off, out_st, route = [POISON_V] * (n + 1), [POISON] * n, [None] * n
    for base, active, workers in _waves(gather_blocks(n) * BLOCK, n, K):  # k_q_col_gather
        wide = {}
        for l in active:
            r = base + l
            o, length = off[r], off[r + 1] - off[r]
            out_off[r], out_st[r] = o, st[r]
            if r + 1 == n:
                out_off[n] = o + length
            if st[r] != OK:
                continue
            if _tag(w, idx[r]) == '"':
                route[r] = string_route(length)
                if length <= K.col_lane:
                    data[o:o + length] = w.string_at(idx[r])
                if length > K.col_wave:
                    wide[l] = (o, length, w.string_at(idx[r]))
            else:
                data[o:o + length] = CW.text(w, idx[r], True)[1]
        _wave_copy(data, wide, workers, K)
    return dict(off=out_off, data=bytes(data), status=out_st, totals=(n, total), trace=dict(route=route))


def _list_elem(w, p, kind):
    """list_elem: (status, value bits / byte length) of the two-word element at p; kind: FLOAT / INT / UINT or "str" """
    tag = _tag(w, p)
    if kind == "str":
        return (OK, w.t[p + 1]) if tag == '"' else (TYPE, 0)
    if tag not in "lud":
        return TYPE, 0
    raw = w.t[p + 1]
    if kind == FLOAT:
        return OK, raw if tag == "d" else CW.f2bits(float(raw - (1 << 64) if tag == "l" and raw >> 63 else raw))
    if tag == "d":
        d = CW.bits2f(raw)
        if d > LW.TWO_63 or d < (-LW.TWO_63 if kind == INT else 0.0):
            return RANGE, 0
        return OK, (1 << 63) if d >= LW.TWO_63 else int(d) & U64
    if (tag == "u" and kind == INT and raw >> 63) or (tag == "l" and kind == UINT and raw >> 63):
        return RANGE, 0
    return OK, raw


def _two_words(w, p):
    return _tag(w, p) in '"lud'


def _lane_measure(w, v, close, kind):
    total = 0
    for k, p in enumerate(range(v + 1, close, 2)):
        st, x = _list_elem(w, p, kind)
        if st != OK:
            return st, 0, 0, k
        total += x
    return OK, (close - v - 1) // 2, total if kind == "str" else 0, None


def _wave_measure(w, v, close, kind, workers, K):
    total = 0
    for si, g in enumerate(range(v + 1, close, 2 * K.step)):
        sts = {}
        for lane in workers:
            p = g + 2 * lane
            if p < close:
                sts[lane] = _list_elem(w, p, kind)
                if K.trust_shifted and _tag(w, p) in "tfn":
                    sts[lane] = (OK, 0)
        bad = [l for l in sts if sts[l][0] != OK]
        if bad:  # one ballot: the lowest lane is the first failing element of the array
            l = max(bad) if K.highest else min(bad)
            return sts[l][0], 0, 0, (si, l)
        total += sum(x for _, x in sts.values())
    return OK, (close - v - 1) // 2, total if kind == "str" else 0, None


def _measure_lists(w, path, mode, K):
    recs = w.records()
    n = len(recs)
    kind = KIND.get(mode, "str")
    idx, cnt, byt, st = [0] * n, [JUNK] * (n + 1), [JUNK] * (n + 1), [0] * n
    route, fail = [None] * n, [None] * n
    for base, active, workers in _waves(_measure_threads(n, K), n, K):
        res, wide = {}, {}
        for l in active:
            r = base + l
            v, s = LW.array_at(w, recs[r], path)
            res[l] = (s, 0, 0)
            if v is None:
                continue
            idx[r], close = v, (w.t[v] & Q.MASK) - 1
            if mode == "list_cvt":  # k_q_list_measure_cvt: the record's lane, whatever the length
                c = b = 0
                p = v + 1
                while s == OK and p < close:
                    s, text = CW.text(w, p, True)
                    b, c, p = b + len(text), c + 1, p + (2 if _two_words(w, p) else 1)
                res[l], route[r] = (s, c, b), LANE
                continue
            words = close - v - 1
            size, unit = (words // 2, 1) if K.by_elems else (words, 2)
            if size <= unit * K.list_lane:
                s, c, b, fail[r] = _lane_measure(w, v, close, kind)
                res[l], route[r] = (s, c, b), LANE
            if size > unit * K.list_wave:
                wide[l], route[r] = (v, close), WIDE
        for l in sorted(wide):
            s, c, b, fail[base + l] = _wave_measure(w, wide[l][0], wide[l][1], kind, workers, K)
            res[l] = (s, c, b)
        for l, (s, c, b) in res.items():
            cnt[base + l], byt[base + l], st[base + l] = (c, b, s) if s == OK else (0, 0, s)
        if base <= n < base + WAVE:
            cnt[n] = byt[n] = 0
    return idx, cnt, byt, st, dict(measure=route, fail=fail)


def _model_numbers(w, path, mode, K):
    idx, cnt, _, st, trace = _measure_lists(w, path, mode, K)
    n, kind = len(st), KIND[mode]
    off, total = _scan(cnt)
    vals = [POISON_V] * total
    out_off, out_st, route = [POISON_V] * (n + 1), [POISON] * n, [None] * n
    for base, active, workers in _waves(gather_blocks(n) * BLOCK, n, K):  # k_q_list_gather_num
        wide = {}
        for l in active:
            r = base + l
            o, c = off[r], off[r + 1] - off[r]
            out_off[r], out_st[r] = o, st[r]
            if r + 1 == n:
                out_off[n] = o + c
            if c <= K.list_lane:
                route[r] = LANE
                for k in range(c):
                    vals[o + k] = _list_elem(w, idx[r] + 1 + 2 * k, kind)[1]
            if c > K.list_wave:
                wide[l], route[r] = (o, c, idx[r]), WIDE
        for j in sorted(wide):
            o, c, v = wide[j]
            for lane in workers:
                for k in range(lane, c, K.step):
                    vals[o + k] = _list_elem(w, v + 1 + 2 * k, kind)[1]
    trace["gather"] = route
    return dict(off=out_off, vals=vals, status=out_st, totals=(n, total), trace=trace)


def _model_list_strings(w, path, mode, K):
    cvt = mode == "list_cvt"
    idx, cnt, byt, st, trace = _measure_lists(w, path, mode, K)
    n = len(st)
    coff, ctot = _scan(cnt)
    boff, btot = _scan(byt)
    soff, data = [POISON_V] * (ctot + 1), bytearray([POISON]) * btot
    out_off, out_st, route, rounds, longs = [POISON_V] * (n + 1), [POISON] * n, [None] * n, {}, [None] * n
    for base, active, workers in _waves(gather_blocks(n) * BLOCK, n, K):  # list_gather_strings
        walks, arrays = {}, {}
        for l in active:
            r = base + l
            o, c = coff[r], coff[r + 1] - coff[r]
            out_off[r], out_st[r] = o, st[r]
            if r + 1 == n:
                out_off[n] = o + c
                soff[o + c] = boff[n]
            if cvt or c <= K.list_lane:
                walks[l], route[r] = [idx[r] + 1, 0, boff[r], c, o], LANE
            if not cvt and c > K.list_wave:
                arrays[l], route[r] = (o, c, idx[r], boff[r]), WIDE
        if active:
            rounds[base // WAVE] = []
        while True:  # every lane walks on to its next long string; the wave copies the waiting lanes' strings; and again
            pend = {}
            for l, s in walks.items():
                while s[1] < s[3] and l not in pend:
                    p, at = s[0], s[2]
                    soff[s[4] + s[1]] = at
                    if _tag(w, p) == '"':
                        length, src = w.t[p + 1], w.string_at(p)
                        if length > K.col_wave:
                            pend[l] = (at, length, src)
                        elif length <= K.col_lane:
                            data[at:at + length] = src
                    else:
                        src = CW.text(w, p, True)[1]
                        length = len(src)
                        data[at:at + length] = src
                    s[0], s[1], s[2] = p + (2 if _two_words(w, p) else 1), s[1] + 1, at + length
            if not pend:
                break
            rounds[base // WAVE].append(tuple(sorted(pend)))
            _wave_copy(data, pend, workers, K)
        for j in sorted(arrays):  # AsString's long arrays: 64 lengths per step, a shuffle scan on a carried base
            o, c, v, at = arrays[j]
            longs[base + j] = []
            for si, g in enumerate(range(0, c, K.step)):
                wide, incl = {}, 0
                for lane in range(WAVE):
                    e = g + lane
                    length = w.t[v + 2 + 2 * e] if e < c and lane in workers else 0
                    incl += length
                    if e < c and lane in workers:
                        mine = at + incl - length
                        soff[o + e] = mine
                        src = w.string_at(v + 1 + 2 * e)
                        if 0 < length <= K.col_lane:
                            data[mine:mine + length] = src
                        if length > K.col_wave:
                            wide[lane] = (mine, length, src)
                            longs[base + j].append((si, lane))
                _wave_copy(data, wide, workers, K)
                if K.carry:
                    at += incl
    trace.update(gather=route, rounds=rounds, long=longs)
    return dict(off=out_off, soff=soff, data=bytes(data), status=out_st, totals=(n, ctot, btot), trace=trace)


def model(doc, path, mode, copy=True, select=None, **mutations):
    """the arrays the device would fetch for `mode` (MODES) at `path`, and the trace; doc: the document, or its walk()"""
    w = walk(doc, copy, select) if isinstance(doc, (bytes, bytearray)) else doc
    K = _K(**dict(_DEFAULTS, **mutations))
    if mode in ("strings", "strings_cvt"):
        return _model_strings(w, path, mode == "strings_cvt", K)
    if mode in KIND:
        return _model_numbers(w, path, mode, K)
    return _model_list_strings(w, path, mode, K)
